"""Retrieval on the auditor (include/omr_gpu.h, "Solve mod 257") measured against the CPU retriever on the same
host, on a 2^20-message board at 50, 250, 1,000 and 4,096 pertinent messages.

    python tools/retrieve_bench.py [--all 1048576] [-k 50 -k 250 -k 1000 -k 4096] [--out profiles/retrieve/time.json]

Per k the system is the board's (k + 5) x k indexed matrix of k random sorted indices with 612 payload columns,
the payload ciphertexts random canonical words (a garbage digest: the solve does the same work and both sides
must still agree bit for bit).
cpu      wall time of omr_retrieve_payloads_indexed (decode on the host's cores, solve on one), CPU_REPEAT runs.
device   wall time of omr_auditor_retrieve_payloads_indexed on the same inputs, copies and synchronisation
         included, after a warm-up, REPEAT runs; every run's payloads are compared with the CPU's.
solve    omr_solve_mod257_device alone on device copies of the same system: HIP events around the call on one
         stream, REPEAT runs after a warm-up, every solution compared with the CPU's.
steps    device milliseconds of one profiled solve per step (omr_solve_profile: events around every kernel,
         so the sum is above the unprofiled solve): panel, row swaps and pivot block, trailing update, back
         substitution.
Every time is reported as min and max / min over its repeats. `faster` says whether the device call's slowest
run beat the CPU call's fastest by more than the CPU's own max / min spread. Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-omr_amd"))
import torch  # noqa: E402  (before libomr_gpu.so: one HIP runtime per process, see tests/conftest.py)

import omr_amd as A  # noqa: E402

REPEAT = 5
SEED = bytes(range(32))


def spread(ts):
    return {"min_s": round(min(ts), 6), "max_over_min": round(max(ts) / min(ts), 3), "runs": len(ts)}


def wall(call):
    t = time.perf_counter()
    r = call()
    return r, time.perf_counter() - t


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int16)).to("cuda:0")


def one(sk, aud, allc, k, cpu_repeat):
    rp = A.RetrievalParams(allc, k)
    rows, per, n_ct = rp.combination_count, rp.cmb_count_per_cipher, rp.cmb_cipher_count
    rng = np.random.default_rng(1000 + k)
    idx = np.sort(rng.choice(allc, k, replace=False))
    cts = rng.integers(0, A.Q2, (n_ct, 2, A.N2), dtype=np.uint64)
    r = A.Retriever(rp, sk)
    out = {"pertinent": k, "rows": rows, "cols": k, "width": A.PAYLOAD_LENGTH, "payload_cts": n_ct}

    cpu_t, want = [], None
    for _ in range(cpu_repeat):
        got, t = wall(lambda: r.decode_combined_payloads_and_solve_indexed(cts, SEED, idx))
        same = want is None or np.array_equal(got, want)
        want = got
        cpu_t.append(t)
        assert same
    out["cpu"] = spread(cpu_t)

    equal = True
    aud.retrieve_payloads_indexed(cts, allc, rows, SEED, idx)  # warm-up: code objects, buffers
    dev_t = []
    for _ in range(REPEAT):
        got, t = wall(lambda: aud.retrieve_payloads_indexed(cts, allc, rows, SEED, idx))
        equal = equal and np.array_equal(got, want)
        dev_t.append(t)
    out["device"] = spread(dev_t)

    # the solve alone, on device copies of the same system
    matrix = A.indexed_weights_at(SEED, rows, idx)
    dec = r.decrypt_decode(cts)
    rhs = np.array([dec[j // per, (j % per) * 612:(j % per + 1) * 612] for j in range(rows)], dtype=np.uint16)
    d_m, d_r = dev(matrix), dev(rhs)
    d_sol = torch.zeros((k, A.PAYLOAD_LENGTH), dtype=torch.int16, device="cuda:0")
    d_st = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def solve():
        aud.solve_mod257_device(d_m.data_ptr(), d_r.data_ptr(), rows, k, A.PAYLOAD_LENGTH, d_sol.data_ptr(), d_st.data_ptr(),
                                st.cuda_stream)

    solve()
    st.synchronize()
    solve_t = []
    for _ in range(REPEAT):
        d_sol.zero_()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            t0.record()
            solve()
            t1.record()
        t1.synchronize()
        solve_t.append(t0.elapsed_time(t1) / 1e3)
        equal = equal and int(d_st.cpu()[0]) == 0 and np.array_equal(d_sol.cpu().numpy().view(np.uint16), want)
    out["solve"] = spread(solve_t)

    aud.solve_profile(True)
    solve()
    ms = aud.solve_profile(False)
    total = sum(ms) or 1.0
    out["steps_ms"] = dict(zip(("panel", "swaps", "update", "back_substitution"), (round(v, 3) for v in ms)))
    out["steps_share"] = dict(zip(("panel", "swaps", "update", "back_substitution"), (round(v / total, 3) for v in ms)))
    out["same_bits"] = bool(equal)
    out["device_over_cpu"] = round(out["device"]["min_s"] / out["cpu"]["min_s"], 4)
    slowest_device = out["device"]["min_s"] * out["device"]["max_over_min"]
    out["faster"] = "device" if slowest_device * out["cpu"]["max_over_min"] < out["cpu"]["min_s"] else (
        "cpu" if out["cpu"]["min_s"] * out["cpu"]["max_over_min"] < out["device"]["min_s"] else "neither")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", type=int, default=1 << 20)
    ap.add_argument("-k", type=int, action="append")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ks = args.k or [50, 250, 1000, 4096]
    if not torch.cuda.is_available():
        raise SystemExit("retrieve_bench: no GPU (this tool measures the device path; it has no fallback)")
    sk = A.SecretKeyPack(42)
    with A.Auditor(sk) as aud:
        results = [one(sk, aud, args.all, k, 5 if k <= 1000 else 2) for k in ks]
    ok = all(r["same_bits"] for r in results)
    line = json.dumps({"all": args.all, "repeat": REPEAT, "geometry": A.solve_geometry(), "results": results, "ok": ok})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
