"""Reference payload weights by seek (include/omr_gpu.h, "Reference payload weights by seek") measured against
the weight table they replace, on a 2^20-message board at 50 and 1,000 pertinent messages.

    python tools/seek_weights_bench.py [--all 1048576] [-k 50 -k 1000] [--out profiles/seek_weights/time.json]

builder  omr_weight_seek_build_device (HIP events around the call, which includes its read-back, and the wall
         clock) and omr_weight_seek_build_cpu (wall clock) against drawing the table with omr_payload_weights
         (wall clock), in the same run; the three agree on the list.
begin    wall time of omr_digest_begin, omr_digest_begin_indexed and omr_digest_begin_seek.
memory   omr_digest_device_bytes of each session after its first 16,384-message host update.
encode   one 16,384-message launch over the same random pertinency words and payloads, in one process:
         omr_encode_payloads_seek_device (encode_payloads_seek_kernel) against omr_encode_payloads_device fed
         omr_payload_weights' table (encode_payloads_kernel). HIP events around each call on one stream,
         alternating, the median of REPEAT after a warm-up, and each kernel's own max / min over its repeats:
         the table kernel's is the noise the ratio is read against.
matrix   omr_payload_weights_at for the recipient's (k + 5) x k matrix (given the seek) against the table draw.
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


def builders(allc, k, st):
    """The two builders and the table draw; returns the table for the encode."""
    rp = A.RetrievalParams(allc, k)
    draws = rp.combination_count * allc
    A.WeightSeek.build(SEED, 1 << 20, device=True, stream=st.cuda_stream)  # warm-up: the kernel's first launch
    dev_ms, dev_wall = [], []
    for _ in range(REPEAT):
        box = {}
        dev_ms.append(event_ms(st, lambda: box.update(s=wall(lambda: A.WeightSeek.build(SEED, draws, device=True,
                                                                                         stream=st.cuda_stream)))))
        dev_wall.append(box["s"][1])
    dev = box["s"][0]
    cpu, cpu_s = wall(lambda: A.WeightSeek.build(SEED, draws))
    table, table_s = wall(lambda: A.payload_weights(SEED, rp))
    return table, dev, {"draws": draws, "rejections": dev.n, "device_event_ms": round(statistics.median(dev_ms), 4),
                        "device_event_max_over_min": round(max(dev_ms) / min(dev_ms), 4),
                        "device_wall_ms": round(statistics.median(dev_wall) * 1e3, 4), "cpu_s": round(cpu_s, 4),
                        "payload_weights_s": round(table_s, 3), "table_bytes": int(table.nbytes),
                        "same_list": bool(dev == cpu)}


def sessions(det, allc, k, clues, payloads):
    """Begin time and footprint of the three session kinds."""
    out = {}
    for name, kw in (("table", {}), ("indexed", {"indexed": True}), ("seek", {"seek": True})):
        dg, t = wall(lambda: det.digest_session(allc, k, INDEX_SEED, SEED, **kw))
        with dg:
            dg.update(clues[0], clues[1], payloads, 0)
            mem = dg.device_bytes()
        out[name] = {"begin_s": round(t, 5), "device_bytes": mem["total"], "weight_bytes": mem["weights"]}
    out["table_over_seek_begin"] = round(out["table"]["begin_s"] / max(out["seek"]["begin_s"], 1e-9), 1)
    return out


def encode(det, allc, k, table, seek, d_pv, d_pay, st):
    rp = A.RetrievalParams(allc, k)
    n_ct, per, cc = rp.cmb_cipher_count, rp.cmb_count_per_cipher, rp.combination_count
    d_w = torch.from_numpy(table.view(np.int16)).to("cuda:0")
    d_a = torch.empty((n_ct, 2, A.N2), dtype=torch.int64, device="cuda:0")
    d_b = torch.empty((n_ct, 2, A.N2), dtype=torch.int64, device="cuda:0")

    def by_table():
        det.encode_payloads_device(d_pv.data_ptr(), d_pay.data_ptr(), PIECE, 0, allc, d_w.data_ptr(), n_ct, per,
                                   d_a.data_ptr(), st.cuda_stream)

    def by_seek():
        det.encode_pertinent_payloads_seek_device(d_pv.data_ptr(), d_pay.data_ptr(), PIECE, 0, allc, SEED, seek, cc, 0,
                                                  n_ct, per, d_b.data_ptr(), st.cuda_stream)

    event_ms(st, by_table), event_ms(st, by_seek)  # warm-up (and the scratch's allocation)
    tab, sk = [], []
    for _ in range(REPEAT):
        tab.append(event_ms(st, by_table))
        sk.append(event_ms(st, by_seek))
    det.check()
    same = bool(torch.equal(d_a, d_b))
    t, s = statistics.median(tab), statistics.median(sk)
    return {"payload_cts": n_ct, "messages": PIECE, "table_kernel_ms": round(t, 4), "seek_kernel_ms": round(s, 4),
            "seek_over_table": round(s / t, 4), "table_max_over_min": round(max(tab) / min(tab), 4),
            "seek_max_over_min": round(max(sk) / min(sk), 4), "same_bits": same}


def matrix(allc, k, seek, table, table_s):
    rp = A.RetrievalParams(allc, k)
    idx = np.sort(np.random.default_rng(k).choice(allc, k, replace=False)).astype(np.uintp)
    m, t_at = wall(lambda: A.payload_weights_at(SEED, allc, rp.combination_count, seek, idx))
    same = bool(np.array_equal(m, table.reshape(-1, allc)[:rp.combination_count][:, idx]))
    return {"rows": int(m.shape[0]), "cols": int(m.shape[1]), "payload_weights_at_s": round(t_at, 6),
            "payload_weights_s": table_s, "same_values": same}


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
        table, seek, b = builders(args.all, k, st)
        r = {"pertinent": k, "builder": b, "encode": encode(det, args.all, k, table, seek, d_pv, d_pay, st)}
        r["matrix"] = matrix(args.all, k, seek, table, b["payload_weights_s"])
        del table
        r["session"] = sessions(det, args.all, k, clues, payloads)
        results.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    det.close()
    ok = all(r["encode"]["same_bits"] and r["builder"]["same_list"] and r["matrix"]["same_values"] for r in results)
    line = json.dumps({"all": args.all, "piece": PIECE, "repeat": REPEAT, "results": results, "ok": ok})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
