"""What a key audit costs (include/omr_gpu.h, "Key audit"), in one process:

  rows     omr_audit_key_rows_device per component on a device-resident key (HIP events around the call)
  device   omr_audit_key on the device-resident key, and omr_audit_key_seeded on device-resident bodies
  host     omr_audit_key from host memory (staged), and omr_audit_key_cpu on 16 threads
  intake   omr_key_validate_device (full key) and omr_key_validate_seeded_device (bodies), beside
           omr_ctx_create_seeded, the cost that intake validation would add to

    python tools/key_audit_bench.py [--sweep] [--out profiles/key_audit/time.json]

--sweep adds the row-range kernels' times over omr_auditor_set_grid (0 = default), with a summary (the
workgroups' global atomics included) and with row_max alone.

Each time is the median of 5 after a warm-up; event times for the row-range kernels, wall clock for the
calls that return when done. Checks that every path gives the CPU's four summaries and prints one JSON line.
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

REPEAT = 5
NAMES = ("bsk1", "ksk", "bsk2", "trace_key")


def wall_ms(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def median_ms(f):
    f()
    return round(statistics.median(wall_ms(f)[0] for _ in range(REPEAT)), 3)


def same(a, b):
    return all(x[k] == y[k] for x, y in zip(a, b) for k in ("rows", "noncanonical", "max_abs_noise", "rows_over",
                                                           "first_row_over")) and \
        all(np.array_equal(x["noise_bits"], y["noise_bits"]) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    torch.cuda.init()
    sk = A.SecretKeyPack(42)
    full = [(int(np.prod(s)), dt) for s, dt in ((A.BSK1_SHAPE, torch.int32), (A.KSK_SHAPE, torch.int32),
                                                (A.BSK2_SHAPE, torch.int64), (A.TK_SHAPE, torch.int64))]
    body = [(int(np.prod(s)), dt) for s, dt in ((A.BSK1_B_SHAPE, torch.int32), (A.KSK_B_SHAPE, torch.int32),
                                                (A.BSK2_B_SHAPE, torch.int64), (A.TK_B_SHAPE, torch.int64))]
    d_key = [torch.empty(n, dtype=dt, device="cuda:0") for n, dt in full]
    d_body = [torch.empty(n, dtype=dt, device="cuda:0") for n, dt in body]
    sk.generate_detection_key_device(7, *[t.data_ptr() for t in d_key])
    sk.generate_seeded_key_device(7, 2026, *[t.data_ptr() for t in d_body])
    torch.cuda.synchronize()
    ptrs = tuple(t.data_ptr() for t in d_key)
    sview = tuple(t.data_ptr() for t in d_body) + (2026,)
    shapes = (A.BSK1_SHAPE, A.KSK_SHAPE, A.BSK2_SHAPE, A.TK_SHAPE)
    host = A.DetectionKey(*[t.cpu().numpy().view(np.uint32 if t.dtype == torch.int32 else np.uint64).reshape(s)
                            for t, s in zip(d_key, shapes)])

    aud = A.Auditor(sk)
    st = torch.cuda.Stream(device="cuda:0")
    init = torch.from_numpy(np.frombuffer(A.key_summary_init_bytes(), np.uint8).copy()).to("cuda:0")

    d_max = torch.zeros(max(k[0] for k in A.KEY_COMPONENTS), dtype=torch.int64, device="cuda:0")

    def rows_ms(c, summary=True):
        d_sum = init.clone()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            t0.record()
            aud.audit_key_rows(c, ptrs[c], 0, A.KEY_COMPONENTS[c][0], d_summary=d_sum.data_ptr() if summary else 0,
                               d_row_max=0 if summary else d_max.data_ptr(), stream=st.cuda_stream)
            t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1), A.key_summary_from_bytes(d_sum.cpu().numpy().tobytes())

    kernels, by_rows = {}, []
    for c in range(4):
        rows_ms(c)
        runs = [rows_ms(c) for _ in range(REPEAT)]
        kernels[NAMES[c]] = round(statistics.median(r[0] for r in runs), 4)
        by_rows.append(runs[-1][1])

    sweep = {}
    if args.sweep:
        for c in range(3):
            for grid in (0, 256, 512, 1024, 2048, 4096, 8192):
                aud.set_grid(grid)
                rows_ms(c)
                sweep[f"{NAMES[c]}_grid{grid}"] = [round(statistics.median(rows_ms(c, f)[0] for _ in range(REPEAT)), 4)
                                                   for f in (True, False)]
        aud.set_grid(0)

    cpu_ms, cpu = wall_ms(lambda: A.audit_key_cpu(sk, host, nthreads=16))
    dev = aud.audit_key(ptrs)
    staged = aud.audit_key(host)
    seeded = aud.audit_seeded_key(sview)
    agree = bool(same(by_rows, cpu) and same(dev, cpu) and same(staged, cpu) and all(s["rows_over"] == 0 for s in cpu + seeded))

    t_create = []
    for _ in range(3):
        ms, det = wall_ms(lambda: A.Detector.from_seeded_key(sview[:4], mask_seed=2026))
        det.close()
        t_create.append(ms)
    out = {
        "kernel_ms": kernels,
        "kernel_rows_per_ms": {NAMES[c]: round(A.KEY_COMPONENTS[c][0] / kernels[NAMES[c]], 1) for c in range(4)},
        "audit_key_device_resident_ms": median_ms(lambda: aud.audit_key(ptrs)),
        "audit_key_seeded_device_bodies_ms": median_ms(lambda: aud.audit_seeded_key(sview)),
        "audit_key_from_host_ms": median_ms(lambda: aud.audit_key(host)),
        "audit_key_cpu_16_threads_ms": round(cpu_ms, 1),
        "validate_device_ms": median_ms(lambda: A.validate_key(ptrs, device=0)),
        "validate_seeded_device_ms": median_ms(lambda: A.validate_key(sview, device=0)),
        "ctx_create_seeded_ms": round(statistics.median(t_create), 2),
        "max_abs_noise": {NAMES[c]: cpu[c]["max_abs_noise"] for c in range(4)},
        "noise_support": {NAMES[c]: A.key_noise_support(c) for c in range(4)},
        "paths_agree": agree,
    }
    if sweep:
        out["grid_sweep_ms_summary_rowmax"] = sweep
    aud.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
