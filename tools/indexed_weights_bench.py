"""Indexed payload weights (include/omr_gpu.h, "Indexed payload weights") measured against the weight table
they replace, on a 2^20-message board at 50 and 1,000 pertinent messages.

    python tools/indexed_weights_bench.py [--all 1048576] [-k 50 -k 1000] [--out profiles/indexed_weights/time.json]

begin    wall time of omr_digest_begin (draws the table on one host thread and uploads it) against
         omr_digest_begin_indexed.
memory   omr_digest_device_bytes of each session after its first 16,384-message host update.
encode   one 16,384-message launch over the same random pertinency words and payloads, in one process:
         omr_encode_payloads_indexed_device (encode_payloads_indexed_kernel) against
         omr_encode_payloads_device fed omr_indexed_weights_table_device's table (encode_payloads_kernel).
         HIP events around each call on one stream, alternating, the median of REPEAT after a warm-up. The
         table kernel's own max / min over its repeats is the noise the ratio is read against.
matrix   omr_indexed_weights_at for the recipient's (k + 5) x k matrix against omr_payload_weights for the
         board, which is what the recipient otherwise waits for.
Prints one JSON line.
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

PIECE, REPEAT, INDEX_SEED = 16384, 7, 99
SEED = bytes(range(32))


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


def wall(call):
    t = time.perf_counter()
    r = call()
    return r, time.perf_counter() - t


def sessions(det, allc, k, clues, payloads):
    """Begin time and footprint of a table session and an indexed session."""
    out = {}
    for name, indexed in (("table", False), ("indexed", True)):
        dg, t = wall(lambda: det.digest_session(allc, k, INDEX_SEED, SEED, indexed=indexed))
        with dg:
            dg.update(clues[0], clues[1], payloads, 0)
            mem = dg.device_bytes()
        out[name] = {"begin_s": round(t, 4), "device_bytes": mem["total"], "weight_bytes": mem["weights"]}
    out["begin_ratio"] = round(out["table"]["begin_s"] / max(out["indexed"]["begin_s"], 1e-9), 1)
    return out


def encode(det, allc, k, d_pv, d_pay, st):
    rp = A.RetrievalParams(allc, k)
    n_ct, per, cc = rp.cmb_cipher_count, rp.cmb_count_per_cipher, rp.combination_count
    d_w = torch.empty(n_ct * per * allc, dtype=torch.int16, device="cuda:0")
    d_a = torch.empty((n_ct, 2, A.N2), dtype=torch.int64, device="cuda:0")
    d_b = torch.empty((n_ct, 2, A.N2), dtype=torch.int64, device="cuda:0")
    fill_ms = event_ms(st, lambda: A.indexed_weights_table_device(SEED, allc, cc, n_ct, per, d_w.data_ptr(), st.cuda_stream))

    def table():
        det.encode_payloads_device(d_pv.data_ptr(), d_pay.data_ptr(), PIECE, 0, allc, d_w.data_ptr(), n_ct, per,
                                   d_a.data_ptr(), st.cuda_stream)

    def indexed():
        det.encode_pertinent_payloads_indexed_device(d_pv.data_ptr(), d_pay.data_ptr(), PIECE, 0, allc, SEED, cc, 0, n_ct,
                                                     per, d_b.data_ptr(), st.cuda_stream)

    event_ms(st, table), event_ms(st, indexed)  # warm-up (and the scratch's allocation)
    tab, ind = [], []
    for _ in range(REPEAT):
        tab.append(event_ms(st, table))
        ind.append(event_ms(st, indexed))
    det.check()
    same = bool(torch.equal(d_a, d_b))
    t, i = statistics.median(tab), statistics.median(ind)
    return {"payload_cts": n_ct, "messages": PIECE, "table_kernel_ms": round(t, 4), "indexed_kernel_ms": round(i, 4),
            "indexed_over_table": round(i / t, 4), "table_max_over_min": round(max(tab) / min(tab), 4),
            "indexed_max_over_min": round(max(ind) / min(ind), 4), "table_fill_device_ms": round(fill_ms, 3),
            "table_bytes": n_ct * per * allc * 2, "same_bits": same}


def matrix(allc, k):
    rp = A.RetrievalParams(allc, k)
    idx = np.sort(np.random.default_rng(k).choice(allc, k, replace=False)).astype(np.uintp)
    m, t_at = wall(lambda: A.indexed_weights_at(SEED, rp.combination_count, idx))
    w, t_tab = wall(lambda: A.payload_weights(SEED, rp))
    return {"rows": int(m.shape[0]), "cols": int(m.shape[1]), "indexed_weights_at_s": round(t_at, 6),
            "payload_weights_s": round(t_tab, 3), "payload_weights_bytes": int(w.nbytes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", type=int, default=1 << 20)
    ap.add_argument("-k", type=int, action="append")
    ap.add_argument("--out")
    args = ap.parse_args()
    torch.cuda.init()
    sk, other = A.SecretKeyPack(42), A.SecretKeyPack(4242)
    clues = other.gen_clues(2, 0, PIECE)
    rng = np.random.default_rng(5)
    payloads = rng.integers(0, 256, (PIECE, A.PAYLOAD_LENGTH)).astype(np.uint16)
    pv = rng.integers(0, A.Q2, (PIECE, 2, A.N2), dtype=np.uint64)
    d_pv = torch.from_numpy(pv.view(np.int64)).to("cuda:0")
    d_pay = torch.from_numpy(payloads.view(np.int16)).to("cuda:0")
    det = device_detector(sk)
    st = torch.cuda.Stream(device="cuda:0")
    st.wait_stream(torch.cuda.current_stream())
    results = []
    for k in args.k or [50, 1000]:
        r = {"pertinent": k, "encode": encode(det, args.all, k, d_pv, d_pay, st)}
        r["session"] = sessions(det, args.all, k, clues, payloads)
        r["matrix"] = matrix(args.all, k)
        results.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    det.close()
    ok = all(r["encode"]["same_bits"] for r in results)
    line = json.dumps({"all": args.all, "piece": PIECE, "repeat": REPEAT, "results": results, "ok": ok})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
