"""Compact ciphertexts (include/omr_gpu.h, "Compact ciphertexts") measured: what the two kernels cost, what a
compact digest read costs, and what compaction does to a real digest's noise.

    python tools/compact_bench.py time  [-n 64 -n 4096 -n 32768] [--grid W] [--out profiles/compact/time.json]
    python tools/compact_bench.py read  [--out profiles/compact/read.json]
    python tools/compact_bench.py noise [--messages 16384] [--out profiles/compact/noise.json]

time   omr_compact_cts_device and omr_compact_expand_device over n device-resident ciphertexts (real detect
       outputs of 64 messages tiled to n, as tools/audit_bench.py reads them) at 20 and 24 bits, and
       omr_audit_device (records + summary) on the same buffer in the same run. HIP events around each
       call on one stream, the median of 5 after a warm-up. GB/s counts the bytes read and written
       (32 KiB + 512 bits bytes per ciphertext); n = 64 is launch-dominated and gets no rate. --grid W
       runs both kernels on W workgroups instead of the default (profiles/compact/grid_sweep.json).
read   one board of 4,096 messages (50 pertinent) in a digest session with a bitmap: omr_digest_read +
       omr_digest_read_bitmap against omr_digest_read_compact at 24 and 20 bits, wall clock, the median
       of 5 after a warm-up, with the bytes each returns.
noise  a board of real detect outputs (50 pertinent at seeded random positions) through a digest session
       with a bitmap: max |r|/q2 of the digest before compaction and after compact + expand at 24, 22 and
       20 bits, next to R(bits)/q2 for the key. Exits non-zero if any ciphertext's residual grows by more
       than R(bits), if any decoded value changes, or if retrieval from an expanded digest differs.
Each mode prints one JSON line.
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

BASE, REPEAT, INDEX_SEED, WEIGHT_SEED = 64, 5, 99, bytes(range(32))
CT_BYTES = 2 * A.N2 * 8


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


def median_ms(st, call):
    event_ms(st, call)  # warm-up
    return statistics.median(event_ms(st, call) for _ in range(REPEAT))


def time_one(det, aud, base, n, st, grid=0):
    reps = (n + BASE - 1) // BASE
    d_cts = torch.from_numpy(base.view(np.int64)).to("cuda:0").repeat(reps, 1, 1)[:n].contiguous()
    d_back = torch.empty_like(d_cts)
    d_rec = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
    d_sum = torch.zeros(440, dtype=torch.uint8, device="cuda:0")
    audit = median_ms(st, lambda: aud.audit_device(d_cts.data_ptr(), n, d_rec.data_ptr(), 0, d_sum.data_ptr(),
                                                   st.cuda_stream))
    out = {"n": n, "audit_device_ms": round(audit, 4)}
    det.set_compact_grid(grid)
    aud.set_grid(grid)  # after the audit's own measurement: from here on it is expand_kernel's grid
    if n >= 1024:
        out["audit_GBps"] = round(n * CT_BYTES / audit / 1e6, 1)
    for bits in (20, 24):
        ctb = A.compact_ct_bytes(bits)
        d_pk = torch.empty(n * ctb, dtype=torch.uint8, device="cuda:0")
        c = median_ms(st, lambda: det.compact_cts_device(d_cts.data_ptr(), n, bits, d_pk.data_ptr(), st.cuda_stream))
        e = median_ms(st, lambda: aud.expand_device(d_pk.data_ptr(), n, bits, d_back.data_ptr(), st.cuda_stream))
        r = {"compact_ms": round(c, 4), "expand_ms": round(e, 4), "compact_over_audit": round(c / audit, 2),
             "expand_over_audit": round(e / audit, 2)}
        if n >= 1024:
            r["compact_GBps"] = round(n * (CT_BYTES + ctb) / c / 1e6, 1)
            r["expand_GBps"] = round(n * (CT_BYTES + ctb) / e / 1e6, 1)
        else:
            r["note"] = "launch-dominated"
        out[f"bits{bits}"] = r
    det.set_compact_grid(0)
    aud.set_grid(0)
    det.check()
    return out


def base_outputs(sk, det):
    other = A.SecretKeyPack(4242)
    ca, cb = other.gen_clues(2, 0, BASE)
    pa, pb = sk.gen_clues(1, 0, 1)
    ca[0], cb[0] = pa[0], pb[0]
    return det.detect_batch(ca, cb)


def run_time(args):
    sk = A.SecretKeyPack(42)
    det = device_detector(sk)
    base = base_outputs(sk, det)
    st = torch.cuda.Stream(device="cuda:0")
    st.wait_stream(torch.cuda.current_stream())
    with A.Auditor(sk) as aud:
        results = [time_one(det, aud, base, n, st, args.grid) for n in (args.n or [64, 4096, 32768])]
    det.close()
    return {"mode": "time", "repeat": REPEAT, "grid": args.grid or "default", "results": results}, 0


def board(sk, n, planted):
    """(clue_a, clue_b, payloads, pertinent positions) of an n-message board."""
    other = A.SecretKeyPack(4242)
    where = np.sort(np.random.default_rng(20261020).choice(n, planted, replace=False))
    ca, cb = other.gen_clues(2, 0, n)
    for g in where:
        pa, pb = sk.gen_clues(1, int(g), 1)
        ca[g], cb[g] = pa[0], pb[0]
    payloads = np.random.default_rng(20261021).integers(0, 256, (n, A.PAYLOAD_LENGTH)).astype(np.uint16)
    return ca, cb, payloads, [int(g) for g in where]


def wall_ms(call):
    call()  # warm-up
    times = []
    for _ in range(REPEAT):
        t = time.perf_counter()
        call()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times)


def run_read(args):
    n, planted = 4096, 50
    sk = A.SecretKeyPack(42)
    det = device_detector(sk)
    ca, cb, payloads, _ = board(sk, n, planted)
    with det.digest_session(n, planted, INDEX_SEED, WEIGHT_SEED) as dg:
        dg.enable_bitmap()
        dg.update(ca, cb, payloads, 0)
        full = wall_ms(lambda: (dg.read(), dg.read_bitmap()))
        idx, pay = dg.read()
        n_ct = idx.shape[0] + pay.shape[0] + dg.read_bitmap().shape[0]
        out = {"mode": "read", "messages": n, "ciphertexts": n_ct, "repeat": REPEAT,
               "read_ms": round(full, 4), "read_bytes": n_ct * CT_BYTES}
        for bits in (24, 20):
            ms = wall_ms(lambda: dg.read_compact(bits, bitmap=True))
            out[f"bits{bits}"] = {"read_compact_ms": round(ms, 4), "read_compact_bytes": n_ct * A.compact_ct_bytes(bits)}
    det.close()
    return out, 0


def run_noise(args):
    n, planted = args.messages, 50
    sk = A.SecretKeyPack(42)
    det = device_detector(sk)
    ca, cb, payloads, where = board(sk, n, planted)
    rp = A.RetrievalParams(n, planted)
    ret = A.Retriever(rp, sk)
    ok = True
    with det.digest_session(n, planted, INDEX_SEED, WEIGHT_SEED) as dg, A.Auditor(sk) as aud:
        dg.enable_bitmap()
        dg.update(ca, cb, payloads, 0)
        idx, pay = dg.read()
        bmp = dg.read_bitmap()
        full = np.concatenate([idx, pay, bmp])
        rec0, dec0, sum0 = aud.audit(full)
        found0, solved0 = ret.decode_digest(idx, pay, WEIGHT_SEED)
        # the bitmap is exact; the index digest may lose an index to a bucket collision, compact or not
        ok = ok and ret.decode_bitmap(bmp) == where
        out = {"mode": "noise", "messages": n, "pertinent": planted, "indices_found": len(found0),
               "index_cts": idx.shape[0], "payload_cts": pay.shape[0],
               "bitmap_cts": bmp.shape[0], "digest_bytes": full.shape[0] * CT_BYTES,
               "max_abs_residual_over_q2": sum0["max_abs_residual"] / A.Q2, "decode_limit": 0.5, "widths": {}}
        for bits in (24, 22, 20):
            packed = np.concatenate(dg.read_compact(bits, bitmap=True))
            rec1, dec1, sum1 = aud.audit_compact(packed, bits)
            back = A.compact_expand_cpu(packed, bits)
            found1, solved1 = ret.decode_digest(back[:idx.shape[0]], back[idx.shape[0]:idx.shape[0] + pay.shape[0]],
                                                WEIGHT_SEED)
            R = A.compact_residual_bound(sk, bits)
            grow = int((rec1["max_abs_residual"].astype(np.int64) - rec0["max_abs_residual"].astype(np.int64)).max())
            same = bool(np.array_equal(dec0, dec1) and found1 == found0 and np.array_equal(solved1, solved0)
                        and ret.decode_bitmap(back[idx.shape[0] + pay.shape[0]:]) == where)
            proven = sum0["max_abs_residual"] + R <= (A.Q2 - 1) // 2
            ok = ok and same and grow <= R
            out["widths"][str(bits)] = {"digest_bytes": int(packed.size), "R_over_q2": R / A.Q2,
                                        "max_abs_residual_over_q2": sum1["max_abs_residual"] / A.Q2,
                                        "largest_increase_over_q2": grow / A.Q2, "increase_over_R": grow / R,
                                        "decoding_proven_by_the_bound": bool(proven), "decoded_and_retrieved_unchanged": same}
    det.close()
    out["ok"] = bool(ok)
    return out, 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("time", "read", "noise"))
    ap.add_argument("-n", type=int, action="append")
    ap.add_argument("--messages", type=int, default=16384)
    ap.add_argument("--grid", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args()
    torch.cuda.init()
    out, rc = {"time": run_time, "read": run_read, "noise": run_noise}[args.mode](args)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
