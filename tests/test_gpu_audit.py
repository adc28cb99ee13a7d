"""The auditor on the GPU (omr_auditor_*, omr_audit_device, omr_audit; include/omr_gpu.h): the crafted,
uniform and out-of-range ciphertexts of audit_cases.py through audit_kernel in every launch shape, against
omr_audit_cpu and the Python statement; the output-pointer combinations; summary accumulation over
calls and streams; and the real pipeline (detect -> audit on one stream with no host copy between, then
a digest session's output). Every comparison is exact integer equality."""
import os
import subprocess

import numpy as np
import pytest

import audit_cases as AC
import product_lib as PL
from product_lib import omr_amd as A

pytestmark = pytest.mark.gpu

N2, Q2 = A.N2, A.Q2
INVALID_ARGUMENT = r"failed \(1\)"
SUMMARY_BYTES = 8 * (5 + A.AUDIT_RESIDUAL_BINS)


class G:
    pass


@pytest.fixture(scope="module")
def g():
    """One pack and auditor, the shared cases, and their expected results (computed once)."""
    import torch
    torch.cuda.init()
    b = G()
    b.sk = A.SecretKeyPack(PL.SK_SEED)
    b.s2 = b.sk.export()["s2"]
    b.cts, b.names = AC.cases()
    b.want = AC.expect(b.cts, b.s2)
    b.cpu = A.audit_cpu(b.sk, b.cts)
    AC.assert_same(b.cpu, b.want, "omr_audit_cpu")
    b.aud = A.Auditor(b.sk, device=0)
    yield b
    b.aud.close()


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, dtype=np.uint64).view(np.int64)).to("cuda:0")  # a writable copy


def subset(b, idx):
    """Expected (records, decoded, summary) of the cases idx."""
    return b.want[0][idx], b.want[1][idx], AC.expect(b.cts[idx], b.s2)[2]


def run_device(aud, cts, records=True, decoded=True, summary=True, stream=None, d_sum=None):
    """omr_audit_device over host ciphertexts uploaded first; returns (records, decoded, summary), None
    where not requested. d_sum: an existing device summary to add into (returned as it is afterwards)."""
    import torch
    n = cts.shape[0]
    d_cts = _dev(cts)
    d_rec = torch.full((n * 16,), 0xA5, dtype=torch.uint8, device="cuda:0") if records else None
    d_dec = torch.full((n, N2), -1, dtype=torch.int16, device="cuda:0") if decoded else None
    if summary and d_sum is None:
        d_sum = torch.zeros(SUMMARY_BYTES, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    aud.audit_device(d_cts.data_ptr(), n, d_rec.data_ptr() if records else 0, d_dec.data_ptr() if decoded else 0,
                     d_sum.data_ptr() if summary else 0, stream.cuda_stream if stream else 0)
    torch.cuda.synchronize()
    return (d_rec.cpu().numpy().view(A.AUDIT_RECORD) if records else None,
            d_dec.cpu().numpy().view(np.uint16) if decoded else None,
            A.Auditor.summary_from_bytes(d_sum.cpu().numpy().tobytes()) if summary else None)


SHAPES = {
    # name: (case indices, grid; 0 = default)
    "n1": ([8], 0),
    "n3_default_grid_idle_workgroups": ([4, 9, 13], 0),
    "n5_grid2_uneven": ([8, 3, 13, 5, 10], 2),   # workgroup 0 takes 3 ciphertexts, workgroup 1 takes 2
    "all14_default_grid": (list(range(14)), 0),
    "all14_grid3": (list(range(14)), 3),          # 5, 5 and 4 per workgroup
    "all14_grid1": (list(range(14)), 1),          # one workgroup reuses its LDS 14 times
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_parity(g, shape):
    idx, grid = SHAPES[shape]
    g.aud.set_grid(grid)
    try:
        got = run_device(g.aud, g.cts[idx])
    finally:
        g.aud.set_grid(0)
    AC.assert_same(got, subset(g, idx), shape)
    AC.assert_same(got[:2], (g.cpu[0][idx], g.cpu[1][idx]), shape + " vs omr_audit_cpu")
    assert int(got[2]["residual_bits"].sum()) == N2 * len(idx)


@pytest.mark.parametrize("staging,idx", [(2, [8, 3, 13, 5, 10]), (0, list(range(14))), (1, [13, 4])])
def test_host_entry_point_staged(g, staging, idx):
    """omr_audit: n = 5 in pieces of 2 (three pieces, the last partial), everything in one piece, and
    pieces of one."""
    g.aud.set_staging(staging)
    try:
        got = g.aud.audit(g.cts[idx])
    finally:
        g.aud.set_staging(0)
    AC.assert_same(got, subset(g, idx), f"staging {staging}")
    AC.assert_same(got, g.aud.audit_cpu(g.cts[idx]), f"staging {staging} vs omr_audit_cpu")


@pytest.mark.parametrize("which", ["records", "decoded", "summary", "all"])
def test_output_pointer_combinations(g, which):
    idx = [1, 4, 13]
    want = subset(g, idx)
    flags = {k: which in (k, "all") for k in ("records", "decoded", "summary")}
    got = run_device(g.aud, g.cts[idx], **flags)
    assert [x is not None for x in got] == [flags["records"], flags["decoded"], flags["summary"]]
    AC.assert_same(got, want, which)


def test_no_output_is_rejected_and_empty_input_is_a_no_op(g):
    import torch
    d_cts = _dev(g.cts[:1])
    d_sum = torch.zeros(SUMMARY_BYTES, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        g.aud.audit_device(d_cts.data_ptr(), 1)
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        g.aud.audit_device(0, 1, d_summary=d_sum.data_ptr())
    with pytest.raises(A.OmrError, match=INVALID_ARGUMENT):
        g.aud.audit_device(d_cts.data_ptr() + 8, 1, d_summary=d_sum.data_ptr())  # not 16-byte aligned
    g.aud.audit_device(0, 0, d_summary=d_sum.data_ptr())
    torch.cuda.synchronize()
    assert not d_sum.cpu().numpy().any()
    rec, dec, summ = g.aud.audit(g.cts[:0])
    assert rec.shape == (0,) and dec.shape == (0, N2) and summ["ciphertexts"] == 0


def test_summary_accumulates_over_calls_and_streams(g):
    import torch
    whole = g.want[2]
    # two calls on one stream
    d_sum = torch.zeros(SUMMARY_BYTES, dtype=torch.uint8, device="cuda:0")
    run_device(g.aud, g.cts[:6], records=False, decoded=False, d_sum=d_sum)
    _, _, got = run_device(g.aud, g.cts[6:], records=False, decoded=False, d_sum=d_sum)
    AC.assert_same((None, None, got), (None, None, whole), "one stream")
    # two calls on two streams into one summary, nothing between them
    d_sum = torch.zeros(SUMMARY_BYTES, dtype=torch.uint8, device="cuda:0")
    d_a, d_b = _dev(g.cts[:9]), _dev(g.cts[9:])
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    g.aud.audit_device(d_a.data_ptr(), 9, d_summary=d_sum.data_ptr(), stream=s1.cuda_stream)
    g.aud.audit_device(d_b.data_ptr(), 5, d_summary=d_sum.data_ptr(), stream=s2.cuda_stream)
    torch.cuda.synchronize()
    got = A.Auditor.summary_from_bytes(d_sum.cpu().numpy().tobytes())
    AC.assert_same((None, None, got), (None, None, whole), "two streams")
    # the host entry point adds into the caller's summary in the same way
    _, _, a = g.aud.audit(g.cts[:6])
    _, _, b = g.aud.audit(g.cts[6:])
    AC.assert_same((None, None, AC.add_summaries(a, b)), (None, None, whole), "omr_audit halves")


def _device_detector(sk):
    """A detector over a device-generated key, as tests/test_gpu_parity.py builds it."""
    import torch
    sizes = [(int(np.prod(A.BSK1_SHAPE)), torch.int32), (int(np.prod(A.KSK_SHAPE)), torch.int32),
             (int(np.prod(A.BSK2_SHAPE)), torch.int64), (int(np.prod(A.TK_SHAPE)), torch.int64)]
    bufs = [torch.empty(n, dtype=dt, device="cuda:0") for n, dt in sizes]
    sk.generate_detection_key_device(PL.KEY_SEED, *[b.data_ptr() for b in bufs])
    return A.Detector.from_device_key(*[b.data_ptr() for b in bufs])


def test_real_pipeline_detect_then_audit_then_digest(g):
    """8 messages, 0, 3 and 6 pertinent: omr_detect_batch_device and omr_audit_device on one stream and
    one buffer; then a digest session over the same messages and the audit of its output.

    Observed on an MI355X (printed below, recorded in DESIGN.md section 1): max |r| / q2 = 4.6e-8 for the
    pertinency vector and 2.2e-5 for its 7-ciphertext digest."""
    import torch
    D, pert = 8, [0, 3, 6]
    other = A.SecretKeyPack(PL.SK2_SEED)
    ca, cb = g.sk.gen_clues(8801, 0, D)
    na, nb = other.gen_clues(8802, 0, D)
    mask = np.zeros(D, bool)
    mask[pert] = True
    ca[~mask], cb[~mask] = na[~mask], nb[~mask]
    det = _device_detector(g.sk)
    try:
        d_ca = torch.from_numpy(ca.view(np.int16)).to("cuda:0")
        d_cb = torch.from_numpy(cb.view(np.int16)).to("cuda:0")
        d_pv = torch.empty((D, 2, N2), dtype=torch.int64, device="cuda:0")
        d_rec = torch.zeros(D * 16, dtype=torch.uint8, device="cuda:0")
        d_dec = torch.zeros((D, N2), dtype=torch.int16, device="cuda:0")
        d_sum = torch.zeros(SUMMARY_BYTES, dtype=torch.uint8, device="cuda:0")
        st = torch.cuda.Stream(device="cuda:0")
        st.wait_stream(torch.cuda.current_stream())
        det.detect_batch_device(d_ca.data_ptr(), d_cb.data_ptr(), D, d_pv.data_ptr(), st.cuda_stream)
        g.aud.audit_device(d_pv.data_ptr(), D, d_rec.data_ptr(), d_dec.data_ptr(), d_sum.data_ptr(), st.cuda_stream)
        det.check(st.cuda_stream)
        rec = d_rec.cpu().numpy().view(A.AUDIT_RECORD)
        dec = d_dec.cpu().numpy().view(np.uint16)
        summ = A.Auditor.summary_from_bytes(d_sum.cpu().numpy().tobytes())
        pv = d_pv.cpu().numpy().view(np.uint64)
        zero, one_hot, other_cls = A.Auditor.classes(rec)
        assert one_hot.tolist() == pert and zero.tolist() == [m for m in range(D) if m not in pert]
        assert other_cls.size == 0 and (summ["one_hot"], summ["zero"], summ["other"]) == (3, 5, 0)
        AC.assert_same((rec, dec, summ), A.audit_cpu(g.sk, pv), "pertinency vector vs omr_audit_cpu")
        pv_noise = summ["max_abs_residual"] / Q2
        print(f"pertinency vector of {D} messages: max |r| / q2 = {pv_noise:.3e}")
        assert summ["max_abs_residual"] * 2 < Q2

        payloads = np.random.default_rng(8803).integers(0, 256, (D, A.PAYLOAD_LENGTH)).astype(np.uint16)
        with det.digest_session(D, len(pert), 8804, bytes(range(32))) as dg:
            dg.update(ca, cb, payloads, 0)
            idx, pay = dg.read()
        digest = np.concatenate([idx, pay])
        rec, dec, summ = g.aud.audit(digest)
        AC.assert_same((rec, dec, summ), A.audit_cpu(g.sk, digest), "digest vs omr_audit_cpu")
        assert np.array_equal(dec, A.Retriever(None, g.sk).decrypt_decode(digest))
        print(f"digest of {D} messages ({digest.shape[0]} ciphertexts): max |r| / q2 = "
              f"{summ['max_abs_residual'] / Q2:.3e}")
        assert summ["max_abs_residual"] / Q2 < 0.5 and summ["max_abs_residual"] * 2 < Q2
        assert summ["ciphertexts"] == digest.shape[0] and dec.any()
    finally:
        det.close()


@pytest.mark.parametrize("extra", [[], ["--session", "7"]], ids=["split", "session"])
def test_native_driver_audit(extra):
    """omr_e2e --audit at its smallest board: exit status 0 and the audit line."""
    subprocess.run(["make", "-s", "-C", os.path.join(PL.ROOT, "tfhe-omr_amd"), "examples"], check=True)
    exe = os.path.join(PL.ROOT, "tfhe-omr_amd", "build", "omr_e2e")
    r = subprocess.run([exe, "-p", "1", "--audit"] + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "audit:" in r.stdout and "All done: 1 pertinent indices and payloads recovered" in r.stdout, r.stdout
