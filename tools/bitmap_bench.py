"""The bitmap digest (include/omr_gpu.h, "Bitmap digest") measured: what it costs and how much noise a
full ciphertext carries.

    python tools/bitmap_bench.py time  [-n 4096 -n 32768] [--out profiles/bitmap/time.json]
    python tools/bitmap_bench.py noise [--out profiles/bitmap/noise.json]

time   omr_encode_bitmap_device over n device-resident pertinency ciphertexts (real detect outputs of 64
       messages tiled to n, as tools/audit_bench.py reads them) as one board of n messages, against
       omr_encode_indices_device for every index ciphertext of the same board on the same buffer. HIP
       events around each call on one stream, the median of 5 after a warm-up; GB/s is the pertinency
       vector's bytes (32 KiB per message) over the bitmap encode's time.
noise  16,384 real detect outputs (one full bitmap ciphertext, 50 of them pertinent at seeded random
       positions) folded into their bitmap ciphertext; the auditor gives E = max |r|/q2 over the
       pertinency ciphertexts and the bitmap ciphertext's max |r|/q2. The derivation bounds the latter
       by 522,240 E + 69 * 255 / q2; exits non-zero if 522,240 E >= 0.5, if the measured value exceeds
       the bound, or if the decoded indices are not the planted ones.
Each mode prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-omr_amd"))
import torch  # noqa: E402  (before libomr_gpu.so: one HIP runtime per process, see tests/conftest.py)

import omr_amd as A  # noqa: E402

BASE, REPEAT, INDEX_SEED = 64, 5, 99
NOISE_FACTOR = 255 * A.N2  # sum_t 2^t over 8 planes x 2,048 coefficients = 522,240


def device_detector(sk):
    sizes = [(int(np.prod(A.BSK1_SHAPE)), torch.int32), (int(np.prod(A.KSK_SHAPE)), torch.int32),
             (int(np.prod(A.BSK2_SHAPE)), torch.int64), (int(np.prod(A.TK_SHAPE)), torch.int64)]
    bufs = [torch.empty(n, dtype=dt, device="cuda:0") for n, dt in sizes]
    sk.generate_detection_key_device(7, *[b.data_ptr() for b in bufs])
    return A.Detector.from_device_key(*[b.data_ptr() for b in bufs])


def event_ms(st, call):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):
        t0.record()
        call()
        t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def time_one(det, base, n, st):
    reps = (n + BASE - 1) // BASE
    d_pv = torch.from_numpy(base.view(np.int64)).to("cuda:0").repeat(reps, 1, 1)[:n].contiguous()
    n_bmp = A.bitmap_ct_count(n)
    n_idx = A.RetrievalParams(n, reps).max_encode_indices_cipher_count
    d_bmp = torch.empty((n_bmp, 2, A.N2), dtype=torch.int64, device="cuda:0")
    d_idx = torch.empty((n_idx, 2, A.N2), dtype=torch.int64, device="cuda:0")

    def bitmap():
        det.encode_bitmap_device(d_pv.data_ptr(), n, 0, n, d_bmp.data_ptr(), st.cuda_stream)

    def indices():
        det.encode_indices_device(d_pv.data_ptr(), n, 0, n, INDEX_SEED, 0, n_idx, d_idx.data_ptr(), st.cuda_stream)

    event_ms(st, bitmap), event_ms(st, indices)  # warm-up (and the scratch's allocation)
    bmp = statistics.median(event_ms(st, bitmap) for _ in range(REPEAT))
    idx = statistics.median(event_ms(st, indices) for _ in range(REPEAT))
    det.check()
    nbytes = n * 2 * A.N2 * 8
    return {"n": n, "bitmap_cts": n_bmp, "index_cts": n_idx, "encode_bitmap_ms": round(bmp, 4),
            "encode_indices_ms": round(idx, 4), "indices_over_bitmap": round(idx / bmp, 2),
            "pv_bytes": nbytes, "bitmap_pv_read_GBps": round(nbytes / bmp / 1e6, 1)}


def run_time(args):
    sk, other = A.SecretKeyPack(42), A.SecretKeyPack(4242)
    ca, cb = other.gen_clues(2, 0, BASE)
    pa, pb = sk.gen_clues(1, 0, 1)
    ca[0], cb[0] = pa[0], pb[0]
    det = device_detector(sk)
    base = det.detect_batch(ca, cb)
    st = torch.cuda.Stream(device="cuda:0")
    st.wait_stream(torch.cuda.current_stream())
    out = {"mode": "time", "repeat": REPEAT, "results": [time_one(det, base, n, st) for n in (args.n or [4096, 32768])]}
    det.close()
    return out, 0


def run_noise(args):
    n, planted = A.BITMAP_MESSAGES_PER_CT, 50
    sk, other = A.SecretKeyPack(42), A.SecretKeyPack(4242)
    where = np.sort(np.random.default_rng(20261020).choice(n, planted, replace=False))
    ca, cb = other.gen_clues(2, 0, n)
    for g in where:
        pa, pb = sk.gen_clues(1, int(g), 1)
        ca[g], cb[g] = pa[0], pb[0]
    det = device_detector(sk)
    pv = det.detect_batch(ca, cb)
    bitmap = det.encode_bitmap(pv, n, 0)
    det.close()
    with A.Auditor(sk) as aud:
        _, _, pv_sum = aud.audit(pv)
        _, decoded, bmp_sum = aud.audit(bitmap)
    found = A.bitmap_indices(decoded, n)
    e = pv_sum["max_abs_residual"] / A.Q2
    measured = bmp_sum["max_abs_residual"] / A.Q2
    bound = NOISE_FACTOR * e + 69 * 255 / A.Q2
    ok = NOISE_FACTOR * e < 0.5 and measured <= bound and found == [int(g) for g in where] \
        and (pv_sum["one_hot"], pv_sum["other"]) == (planted, 0)
    out = {"mode": "noise", "messages": n, "pertinent": planted, "found": len(found),
           "classes": {"one_hot": pv_sum["one_hot"], "zero": pv_sum["zero"], "other": pv_sum["other"]},
           "E_max_abs_residual_over_q2": e, "bound_522240_E": NOISE_FACTOR * e,
           "bitmap_max_abs_residual_over_q2": measured, "measured_over_bound": measured / bound,
           "decode_limit": 0.5, "ok": bool(ok)}
    return out, 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("time", "noise"))
    ap.add_argument("-n", type=int, action="append")
    ap.add_argument("--out")
    args = ap.parse_args()
    torch.cuda.init()
    out, rc = (run_time if args.mode == "time" else run_noise)(args)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
