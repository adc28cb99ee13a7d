"""The check "did the detector produce the right pertinency vector" for n device-resident ciphertexts,
both ways, in one process:

  device  omr_audit_device on the buffer where it is (records + summary; and with the decoded values)
  host    the existing path: copy the buffer to the host, omr_decrypt_decode on the host's threads

    python tools/audit_bench.py [-n 4096] [--out FILE.json]

The ciphertexts are real detect outputs (64 messages, message 0 pertinent, tiled to n on the device).
Device times are HIP events around the call, host times wall clock; each the median of 5 after a
warm-up. Checks that both paths classify every ciphertext alike and prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-omr_amd"))
import torch  # noqa: E402  (before libomr_gpu.so: one HIP runtime per process, see tests/conftest.py)

import omr_amd as A  # noqa: E402

BASE, REPEAT = 64, 5


def device_detector(sk):
    sizes = [(int(np.prod(A.BSK1_SHAPE)), torch.int32), (int(np.prod(A.KSK_SHAPE)), torch.int32),
             (int(np.prod(A.BSK2_SHAPE)), torch.int64), (int(np.prod(A.TK_SHAPE)), torch.int64)]
    bufs = [torch.empty(n, dtype=dt, device="cuda:0") for n, dt in sizes]
    sk.generate_detection_key_device(7, *[b.data_ptr() for b in bufs])
    return A.Detector.from_device_key(*[b.data_ptr() for b in bufs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-n", type=int, default=4096)
    ap.add_argument("--out")
    args = ap.parse_args()
    n = args.n
    torch.cuda.init()
    sk, other = A.SecretKeyPack(42), A.SecretKeyPack(4242)
    ca, cb = other.gen_clues(2, 0, BASE)
    pa, pb = sk.gen_clues(1, 0, 1)
    ca[0], cb[0] = pa[0], pb[0]
    det = device_detector(sk)
    base = det.detect_batch(ca, cb)
    det.close()
    reps = (n + BASE - 1) // BASE
    d_pv = torch.from_numpy(base.view(np.int64)).to("cuda:0").repeat(reps, 1, 1)[:n].contiguous()
    pertinent = np.arange(n) % BASE == 0

    aud = A.Auditor(sk)
    ret = A.Retriever(None, sk)
    d_rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
    d_dec = torch.zeros((n, A.N2), dtype=torch.int16, device="cuda:0")
    st = torch.cuda.Stream(device="cuda:0")
    st.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()

    def device_ms(with_decoded):
        d_sum = torch.zeros(440, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            t0.record()
            aud.audit_device(d_pv.data_ptr(), n, d_rec.data_ptr(), d_dec.data_ptr() if with_decoded else 0,
                             d_sum.data_ptr(), st.cuda_stream)
            t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1), d_sum

    def host_ms():
        t = time.perf_counter()
        pv = d_pv.cpu().numpy().view(np.uint64)
        t_copy = time.perf_counter()
        dec = ret.decrypt_decode(pv)
        return (time.perf_counter() - t) * 1e3, (t_copy - t) * 1e3, dec

    device_ms(True), host_ms()  # warm-up
    dev = [device_ms(False)[0] for _ in range(REPEAT)]
    dev_dec = [device_ms(True)[0] for _ in range(REPEAT)]
    host = [host_ms()[:2] for _ in range(REPEAT)]
    _, d_sum = device_ms(True)
    _, _, dec = host_ms()

    rec = d_rec.cpu().numpy().view(A.AUDIT_RECORD)
    summ = A.Auditor.summary_from_bytes(d_sum.cpu().numpy().tobytes())
    zero, one_hot, oth = A.Auditor.classes(rec)
    host_one_hot = (dec[:, 0] == 1) & (np.count_nonzero(dec, axis=1) == 1)
    host_zero = ~dec.any(axis=1)
    agree = bool(np.array_equal(np.nonzero(host_one_hot)[0], one_hot) and np.array_equal(np.nonzero(host_zero)[0], zero)
                 and np.array_equal(d_dec.cpu().numpy().view(np.uint16), dec.astype(np.uint16))
                 and np.array_equal(one_hot, np.nonzero(pertinent)[0]) and oth.size == 0)
    aud.close()
    dev_med, host_med = statistics.median(dev), statistics.median(h[0] for h in host)
    out = {"n": n, "audit_device_ms": round(dev_med, 4), "audit_device_with_decoded_ms": round(statistics.median(dev_dec), 4),
           "host_check_ms": round(host_med, 3), "host_copy_ms": round(statistics.median(h[1] for h in host), 3),
           "host_threads": min(16, os.cpu_count() or 1), "ratio_host_over_device": round(host_med / dev_med, 2),
           "classes": {"one_hot": summ["one_hot"], "zero": summ["zero"], "other": summ["other"]},
           "max_abs_residual_over_q2": summ["max_abs_residual"] / A.Q2, "paths_agree": agree}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
