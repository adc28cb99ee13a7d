"""Compact ciphertexts on the GPU (include/omr_gpu.h, "Compact ciphertexts"): compact_kernel through
omr_compact_cts_device / omr_compact_cts and expand_kernel through omr_compact_expand_device /
omr_audit_compact against the CPU statement (which test_compact_host.py pins to the Python-integer model),
byte for byte, for every width and launch shape; the crafted inputs of compact_model.py against the CPU statement
and the model: coefficients on either side of a rounding step, where the device's FP64 quotient estimate and its
correction decide, and packed streams with boundary values at every kind of stream-word position; then one real
board through a digest session:
omr_digest_read_compact, retrieval from the expanded digest, the residual increase against R(bits), and the
session call's argument rules. Every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import audit_cases as AC
import compact_model as M
import product_lib as PL
import test_gpu_digest_session as DS
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu

N2, Q2 = A.N2, A.Q2
INVALID_ARGUMENT = r"failed \(1\)"
ALL_BITS = list(range(16, 33))
MANY = 300  # uniform ciphertexts (9.4 MiB): more than any grid used below, in uneven shares


class G:
    pass


@pytest.fixture(scope="module")
def g():
    """One detector and auditor, the 14 shared cases and MANY uniform ciphertexts on host and device."""
    import torch
    torch.cuda.init()
    a, _, dk = PL.keys()
    b = G()
    b.sk = a
    b.det = A.Detector(dk)
    b.aud = A.Auditor(a, device=0)
    b.cts, b.names = AC.cases()
    b.d_cts = dev(b.cts)
    b.many = np.random.default_rng(20261021).integers(0, Q2, (MANY, 2, N2), dtype=np.uint64)
    b.many.setflags(write=False)
    b.d_many = dev(b.many)
    b.cpu = {}  # bits -> omr_compact_cts_cpu of the 14 cases
    yield b
    b.aud.close()
    b.det.close()


def dev(x):
    import torch
    return torch.from_numpy(np.array(x).view(np.int64 if x.dtype == np.uint64 else np.uint8)).to("cuda:0")


def cpu_cases(b, bits):
    if bits not in b.cpu:
        b.cpu[bits] = A.compact_cts_cpu(b.cts, bits)
    return b.cpu[bits]


def compact_device(b, d_cts, n, bits, stream=None):
    """omr_compact_cts_device into a buffer pre-filled with 0xA5 and with a guard ciphertext behind it."""
    import torch
    ctb = 512 * bits
    d_out = torch.full(((n + 1) * ctb,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    b.det.compact_cts_device(d_cts.data_ptr(), n, bits, d_out.data_ptr(), stream.cuda_stream if stream else 0)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[n * ctb:] == 0xA5).all(), "wrote beyond the last ciphertext"
    return out[:n * ctb].reshape(n, ctb)


def expand_device(b, packed, bits):
    """omr_compact_expand_device of host compact ciphertexts, with a guard ciphertext behind the output."""
    import torch
    n = packed.shape[0]
    d_in = dev(packed.reshape(-1))
    d_out = torch.full(((n + 1), 2, N2), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    b.aud.expand_device(d_in.data_ptr(), n, bits, d_out.data_ptr())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint64)
    assert (out[n] == 2**64 - 1).all(), "wrote beyond the last ciphertext"
    return out[:n]


@pytest.mark.parametrize("bits", ALL_BITS)
def test_every_width_on_the_shared_cases(g, bits):
    """The 14 cases at one width: device and host entry of compact, device expand, all against the CPU."""
    want = cpu_cases(g, bits)
    assert np.array_equal(compact_device(g, g.d_cts, 14, bits), want)
    assert np.array_equal(g.det.compact_cts(g.cts, bits), want)
    assert np.array_equal(expand_device(g, want, bits), A.compact_expand_cpu(want, bits))


@pytest.mark.parametrize("bits", [16, 21, 32])
def test_launch_shapes(g, bits):
    """n = 1; n = 3 through the host entry staged by 2 (the last piece short); a grid of 3 striding over 14
    (5, 5 and 4 per workgroup) and of 1 (one workgroup reuses its LDS 14 times), for both kernels."""
    want = cpu_cases(g, bits)
    assert np.array_equal(compact_device(g, g.d_cts[13:], 1, bits), want[13:])
    assert np.array_equal(expand_device(g, want[8:9], bits), A.compact_expand_cpu(want[8:9], bits))
    g.det.set_compact_staging(2)
    try:
        assert np.array_equal(g.det.compact_cts(g.cts[[4, 13, 9]], bits), want[[4, 13, 9]])
    finally:
        g.det.set_compact_staging(0)
    back = A.compact_expand_cpu(want, bits)
    for grid in (3, 1):
        g.det.set_compact_grid(grid)
        g.aud.set_grid(grid)
        try:
            assert np.array_equal(compact_device(g, g.d_cts, 14, bits), want), grid
            assert np.array_equal(expand_device(g, want, bits), back), grid
        finally:
            g.det.set_compact_grid(0)
            g.aud.set_grid(0)


@pytest.mark.parametrize("bits", [20, 24])
def test_more_ciphertexts_than_the_grid(g, bits):
    """300 uniform ciphertexts over a grid of 64 (44 shares of 5 and 20 of 4, on a stream of the caller's)
    and over the default grid; the expansion of all of them likewise; 70 through the host entry."""
    import torch
    want = A.compact_cts_cpu(g.many, bits)
    st = torch.cuda.Stream(device="cuda:0")
    g.det.set_compact_grid(64)
    g.aud.set_grid(64)
    try:
        assert np.array_equal(compact_device(g, g.d_many, MANY, bits, stream=st), want)
        got = expand_device(g, want, bits)
    finally:
        g.det.set_compact_grid(0)
        g.aud.set_grid(0)
    assert np.array_equal(got, A.compact_expand_cpu(want, bits))
    assert np.array_equal(compact_device(g, g.d_many, MANY, bits), want)
    assert np.array_equal(g.det.compact_cts(g.many[:70], bits), want[:70])


@pytest.mark.parametrize("bits", ALL_BITS)
def test_rounding_steps_on_the_device(g, bits):
    """compact_rescale as the device compiles it, on either side of a step: the three crafted ciphertexts (steps
    y = 1, Q / 2, Q - 1 and Q at the thread and register edges, q2 - 1 wrapping to 0) and the ladder (all 2,048
    coefficients one below, and at, a step of their own, y from 1 to Q), through the device and the host entry,
    by one workgroup and by the default grid, against the CPU statement and the Python-integer model."""
    cts, pairs = M.crafted_cts(bits)
    want = A.compact_cts_cpu(cts, bits)
    for i, (ca, cb) in enumerate(pairs):
        assert want[i].tobytes() == M.compact_coefficients(ca, cb, bits), i
    d_cts = dev(cts)
    for grid in (1, 0):
        g.det.set_compact_grid(grid)
        try:
            got_device = compact_device(g, d_cts, len(pairs), bits)
            got_host = g.det.compact_cts(cts, bits)
        finally:
            g.det.set_compact_grid(0)
        assert np.array_equal(got_device, want), (grid, np.argwhere(got_device != want)[:5])
        assert np.array_equal(got_host, want), grid


@pytest.mark.parametrize("bits", ALL_BITS)
def test_expand_boundary_values_on_the_device(g, bits):
    """expand_kernel on streams with y = 0, 1, Q / 2 and Q - 1 at the first and the last value and at values that
    end on, start on and straddle a 32-bit stream word, against omr_compact_expand_cpu and the model."""
    packed = M.expand_streams(bits)
    want = A.compact_expand_cpu(packed, bits)
    for i in range(packed.shape[0]):
        assert np.array_equal(want[i], M.expand(packed[i].tobytes(), bits)), i
    assert int(want.max()) < Q2
    for grid in (1, 0):
        g.aud.set_grid(grid)
        try:
            got = expand_device(g, packed, bits)
        finally:
            g.aud.set_grid(0)
        assert np.array_equal(got, want), (grid, np.argwhere(got != want)[:5])


@pytest.mark.parametrize("bits,staging", [(24, 0), (20, 2), (16, 1), (32, 0)])
def test_audit_compact_equals_audit_of_the_cpu_expansion(g, bits, staging):
    packed = cpu_cases(g, bits)[[8, 3, 13, 5, 10]] if staging else cpu_cases(g, bits)
    back = A.compact_expand_cpu(packed, bits)
    g.aud.set_staging(staging)
    try:
        got = g.aud.audit_compact(packed, bits)
        AC.assert_same(got, g.aud.audit(back), f"omr_audit_compact vs omr_audit at {bits} bits")
    finally:
        g.aud.set_staging(0)
    AC.assert_same(got, A.audit_cpu(g.sk, back), f"omr_audit_compact vs omr_audit_cpu at {bits} bits")
    assert got[2]["ciphertexts"] == packed.shape[0]


def test_argument_errors_before_anything_is_enqueued(g):
    import torch
    d_out = torch.full((512 * 32,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_back = torch.full((2, N2), -1, dtype=torch.int64, device="cuda:0")
    p_in, p_out, p_back = g.d_cts.data_ptr(), d_out.data_ptr(), d_back.data_ptr()
    for bits in (15, 33, 0):
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            g.det.compact_cts_device(p_in, 1, bits, p_out)
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            g.aud.expand_device(p_out, 1, bits, p_back)
        assert A.lib().omr_compact_cts(g.det.handle, g.cts.ctypes.data, 1, bits, p_out) == 1
        assert A.lib().omr_audit_compact(g.aud._h, g.cts.ctypes.data, 1, bits, None, None,
                                         C.addressof(A._AuditSummary())) == 1
    for args in ((0, 1, 24, p_out), (p_in, 1, 24, 0), (p_in + 8, 1, 24, p_out), (p_in, 1, 24, p_out + 4)):
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            g.det.compact_cts_device(*args)
    for args in ((0, 1, 24, p_back), (p_out, 1, 24, 0), (p_out + 8, 1, 24, p_back), (p_out, 1, 24, p_back + 8)):
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            g.aud.expand_device(*args)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):  # no output requested
        A._check(A.lib().omr_audit_compact(g.aud._h, g.cts.ctypes.data, 1, 24, None, None, None), "omr_audit_compact")
    # n = 0 does nothing
    g.det.compact_cts_device(0, 0, 24, 0)
    g.aud.expand_device(0, 0, 24, 0)
    assert g.det.compact_cts(g.cts[:0], 24).shape == (0, 512 * 24)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xA5).all() and (d_back.cpu().numpy() == -1).all()


# ---- one real board: the geometry of test_gpu_digest_session.py, with a bitmap ---------------------

@pytest.fixture(scope="module")
def board(g):
    """The 300-message board of the digest-session tests through one session with a bitmap: the full
    digest before and after the compact reads, the compact reads at 24 and 20 bits, and the audit of the
    full digest; the session stays open for the tests that need it."""
    b = G()
    b.ca, b.cb, b.payloads = DS.board()
    b.rp = A.RetrievalParams(DS.ALL, len(DS.PERTINENT))
    b.dg = g.det.digest_session(DS.ALL, len(DS.PERTINENT), DS.INDEX_SEED, DS.WEIGHT_SEED)
    b.dg.enable_bitmap()
    b.dg.update(b.ca, b.cb, b.payloads, 0)
    b.idx, b.pay = b.dg.read()
    b.bmp = b.dg.read_bitmap()
    b.compact = {bits: b.dg.read_compact(bits, bitmap=True) for bits in (24, 20)}
    b.idx_after, b.pay_after = b.dg.read()
    b.bmp_after = b.dg.read_bitmap()
    b.full = np.concatenate([b.idx, b.pay, b.bmp])
    b.audit = A.audit_cpu(g.sk, b.full)
    yield b
    b.dg.close()


@pytest.mark.parametrize("bits", [24, 20])
def test_digest_read_compact_equals_the_cpu_statement(g, board, bits):
    idx, pay, bmp = board.compact[bits]
    assert idx.shape == (5, 512 * bits) and pay.shape == (4, 512 * bits) and bmp.shape == (1, 512 * bits)
    assert np.array_equal(idx, A.compact_cts_cpu(board.idx, bits))
    assert np.array_equal(pay, A.compact_cts_cpu(board.pay, bits))
    assert np.array_equal(bmp, A.compact_cts_cpu(board.bmp, bits))


def test_the_running_digest_is_not_modified(board):
    assert np.array_equal(board.idx_after, board.idx) and np.array_equal(board.pay_after, board.pay)
    assert np.array_equal(board.bmp_after, board.bmp)


@pytest.mark.parametrize("bits", [24, 20])
def test_retrieval_from_the_expanded_digest(g, board, bits):
    """Expanded on the device, the compact digest retrieves exactly what the full digest retrieves, and no
    ciphertext's largest residual grows by more than R(bits)."""
    packed = np.concatenate(board.compact[bits])
    back = expand_device(g, packed, bits)
    assert np.array_equal(back, A.compact_expand_cpu(packed, bits))
    idx, pay, bmp = back[:5], back[5:9], back[9:]
    r = A.Retriever(board.rp, g.sk)
    want_found, want_solved = r.decode_digest(board.idx, board.pay, DS.WEIGHT_SEED)
    found, solved = r.decode_digest(idx, pay, DS.WEIGHT_SEED)
    assert found == want_found == list(DS.PERTINENT)
    assert np.array_equal(solved, want_solved) and np.array_equal(solved, board.payloads[list(DS.PERTINENT)])
    assert r.decode_bitmap(bmp) == r.decode_bitmap(board.bmp) == list(DS.PERTINENT)
    rec, dec, summ = g.aud.audit_compact(packed, bits)
    AC.assert_same((rec, dec, summ), A.audit_cpu(g.sk, back), "audit of the compact digest")
    assert np.array_equal(dec, board.audit[1])
    R = A.compact_residual_bound(g.sk, bits)
    grow = rec["max_abs_residual"].astype(np.int64) - board.audit[0]["max_abs_residual"].astype(np.int64)
    print(f"{bits} bits: digest max |r| / q2 {board.audit[2]['max_abs_residual'] / Q2:.3e} -> "
          f"{summ['max_abs_residual'] / Q2:.3e}; largest increase / q2 {int(grow.max()) / Q2:.3e}, R / q2 {R / Q2:.3e}")
    assert int(grow.max()) <= R
    assert board.audit[2]["max_abs_residual"] + R <= (Q2 - 1) // 2


def test_session_argument_rules(g, board):
    """The argument rules of omr_digest_read_compact. Its poisoning rules are omr_digest_read's (the same
    check on entry, the same hand-off error taken after the synchronisation); only a device failure
    poisons a session, and no test causes one."""
    L = A.lib()
    buf = np.zeros(5 * 512 * 32, np.uint8)
    for bits in (15, 33):
        assert L.omr_digest_read_compact(board.dg._h, bits, buf.ctypes.data, None, None) == 1
    assert not buf.any()
    # any pointer may be NULL, all of them too
    assert L.omr_digest_read_compact(board.dg._h, 24, None, None, None) == 0
    assert L.omr_digest_read_compact(board.dg._h, 24, None, None, buf.ctypes.data) == 0
    assert np.array_equal(buf[:512 * 24], board.compact[24][2][0])
    assert L.omr_digest_read_compact(board.dg._h, 24, buf.ctypes.data, None, None) == 0
    assert np.array_equal(buf[:5 * 512 * 24].reshape(5, -1), board.compact[24][0])
    # a session without a bitmap: the bitmap pointer is an argument error, the session stays usable
    with g.det.digest_session(DS.ALL, len(DS.PERTINENT), DS.INDEX_SEED, DS.WEIGHT_SEED) as dg:
        with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
            dg.read_compact(24, bitmap=True)
        idx, pay = dg.read_compact(24)
        zero = A.compact_cts_cpu(np.zeros((1, 2, N2), np.uint64), 24)[0]
        assert not zero.any() and not idx.any() and not pay.any()  # an empty digest compacts to zeros
        assert dg.info()["messages"] == 0
