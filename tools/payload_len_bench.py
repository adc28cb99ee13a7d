"""The payload encode with the length as an argument (include/omr_gpu.h, "Payload length as a board
parameter") measured against the kernel it generalises, and what a length costs.

    python tools/payload_len_bench.py [--out profiles/payload_len/time.json]

same612  one 16,384-message launch at L = 612 with 2 combinations per ciphertext, at 28 and at 503
         ciphertexts (50 and 1,000 pertinent messages): omr_encode_payloads_indexed_len_device
         (encode_payloads_indexed_len_kernel) against omr_encode_payloads_indexed_device
         (encode_payloads_indexed_kernel) over the same random pertinency words and payloads, in one process.
         HIP events around each call on one stream, alternating, the median of REPEAT after a warm-up. The
         yardstick is the existing kernel: its own max / min over its repeats is the noise the ratio is read
         against. The two outputs must be the same bits.
lengths  the time of one such launch at L = 64, 128, 2048 and 16384 with 55 combinations, at the layout of
         omr_get_payload_layout, with the ciphertext count of each.
Prints one JSON line.
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

PIECE, REPEAT, ALL = 16384, 7, 1 << 20
SEED = bytes(range(32))
LENGTHS = (64, 128, 2048, 16384)


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


def payloads_of(L):
    pay = np.random.default_rng(L).integers(0, 256, (PIECE, L)).astype(np.uint16)
    return torch.from_numpy(pay.view(np.int16)).to("cuda:0")


def same612(det, k, d_pv, d_pay, st):
    rp = A.RetrievalParams(ALL, k)
    n_ct, per, cc = rp.cmb_cipher_count, rp.cmb_count_per_cipher, rp.combination_count
    d_a = torch.empty((n_ct, 2, A.N2), dtype=torch.int64, device="cuda:0")
    d_b = torch.empty((n_ct, 2, A.N2), dtype=torch.int64, device="cuda:0")

    def indexed():
        det.encode_pertinent_payloads_indexed_device(d_pv.data_ptr(), d_pay.data_ptr(), PIECE, 0, ALL, SEED, cc, 0, n_ct,
                                                     per, d_a.data_ptr(), st.cuda_stream)

    def by_len():
        det.encode_pertinent_payloads_indexed_len_device(d_pv.data_ptr(), d_pay.data_ptr(), PIECE, 0, ALL, SEED, cc,
                                                         A.PAYLOAD_LENGTH, per, 0, n_ct, d_b.data_ptr(), st.cuda_stream)

    event_ms(st, indexed), event_ms(st, by_len)  # warm-up (and the scratch's allocation)
    ind, ln = [], []
    for _ in range(REPEAT):
        ind.append(event_ms(st, indexed))
        ln.append(event_ms(st, by_len))
    det.check()
    i, n = statistics.median(ind), statistics.median(ln)
    return {"pertinent": k, "payload_cts": n_ct, "cmb_per_ct": per, "messages": PIECE, "indexed_kernel_ms": round(i, 4),
            "len_kernel_ms": round(n, 4), "len_over_indexed": round(n / i, 4),
            "indexed_max_over_min": round(max(ind) / min(ind), 4), "len_max_over_min": round(max(ln) / min(ln), 4),
            "same_bits": bool(torch.equal(d_a, d_b))}


def one_length(det, L, d_pv, st):
    ly = A.PayloadLayout.of(50, L)
    d_pay = payloads_of(L)
    d_out = torch.empty((ly.payload_ct, 2, A.N2), dtype=torch.int64, device="cuda:0")

    def call():
        det.encode_pertinent_payloads_indexed_len_device(d_pv.data_ptr(), d_pay.data_ptr(), PIECE, 0, ALL, SEED,
                                                         ly.combination_count, L, ly.cmb_count_per_cipher, 0, ly.payload_ct,
                                                         d_out.data_ptr(), st.cuda_stream)

    event_ms(st, call)
    ms = [event_ms(st, call) for _ in range(REPEAT)]
    det.check()
    return {"payload_len": L, "combination_count": ly.combination_count, "cmb_per_ct": ly.cmb_count_per_cipher,
            "stripes": ly.stripes, "payload_cts": ly.payload_ct, "launch_ms": round(statistics.median(ms), 4),
            "max_over_min": round(max(ms) / min(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    torch.cuda.init()
    pv = np.random.default_rng(5).integers(0, A.Q2, (PIECE, 2, A.N2), dtype=np.uint64)
    d_pv = torch.from_numpy(pv.view(np.int64)).to("cuda:0")
    det = device_detector(A.SecretKeyPack(42))
    st = torch.cuda.Stream(device="cuda:0")
    st.wait_stream(torch.cuda.current_stream())
    d_pay = payloads_of(A.PAYLOAD_LENGTH)
    same = [same612(det, k, d_pv, d_pay, st) for k in (50, 1000)]
    for r in same:
        print(json.dumps(r), file=sys.stderr, flush=True)
    del d_pay
    lengths = []
    for L in LENGTHS:
        lengths.append(one_length(det, L, d_pv, st))
        print(json.dumps(lengths[-1]), file=sys.stderr, flush=True)
    det.close()
    ok = all(r["same_bits"] for r in same)
    line = json.dumps({"all": ALL, "piece": PIECE, "repeat": REPEAT, "same612": same, "lengths": lengths, "ok": ok})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
