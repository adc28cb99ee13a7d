"""The seeded detection key (include/omr_gpu.h, "Seeded detection key") measured: what expansion costs
next to the key conversion it feeds.

    python tools/seeded_key_bench.py [--out profiles/seeded/seeded_key.json]

expand_device_ms   omr_expand_detection_key_device with the bodies already in device memory (the call
                   returns after its stream has completed, so a host clock around it measures the device
                   work plus one launch round trip), median of 5 after a warm-up; GB/s is the expanded key's
                   bytes over that time.
create_full_ms     omr_ctx_create from a full key in host memory (362.6 MiB cross PCIe), and
create_seeded_ms   omr_ctx_create_seeded from the bodies in host memory (146.0 MiB cross PCIe, expanded on
                   the device), alternating in the same process, median of 5 after a warm-up of each.
The byte counts come from the arrays. Prints one JSON line; no thresholds.
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

REPEAT, SK_SEED, KEY_SEED, MASK_SEED = 5, 42, 7, 2026


def wall_ms(call):
    torch.cuda.synchronize()
    t = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def dev(a):
    signed = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.reshape(-1).view(signed)).to("cuda:0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded", "seeded_key.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("seeded_key_bench: no GPU")
    pack = A.SecretKeyPack(SK_SEED)
    sk = pack.generate_seeded_key(KEY_SEED, MASK_SEED, nthreads=16)
    full = sk.expand(nthreads=16)
    d_bodies = [dev(a) for a in (sk.bsk1_b, sk.ksk_b, sk.bsk2_b, sk.trace_key_b)]
    d_full = [torch.empty(a.size, dtype={4: torch.int32, 8: torch.int64}[a.dtype.itemsize], device="cuda:0")
              for a in (full.bsk1, full.ksk, full.bsk2, full.trace_key)]

    def expand():
        A.expand_detection_key_device([b.data_ptr() for b in d_bodies], MASK_SEED, *[o.data_ptr() for o in d_full])

    expand()  # warm-up (code object load), and the check that what is timed is the right key
    for a, o in zip((full.bsk1, full.ksk, full.bsk2, full.trace_key), d_full):
        if not np.array_equal(o.cpu().numpy().view(a.dtype).reshape(a.shape), a):
            sys.exit("seeded_key_bench: device expansion differs from host expansion")
    expand_ms = [wall_ms(expand) for _ in range(REPEAT)]
    del d_full, d_bodies

    def create(seeded):
        holder = []
        ms = wall_ms(lambda: holder.append(A.Detector.from_seeded_key(sk) if seeded else A.Detector(full)))
        holder[0].close()
        return ms

    create(False), create(True)  # warm-up of each path
    full_ms, seeded_ms = [], []
    for _ in range(REPEAT):
        full_ms.append(create(False))
        seeded_ms.append(create(True))
    e, f, s = statistics.median(expand_ms), statistics.median(full_ms), statistics.median(seeded_ms)
    res = {
        "tool": "seeded_key_bench", "device": torch.cuda.get_device_name(0), "repeat": REPEAT,
        "seeded_key_bytes": sk.size(), "full_key_bytes": full.size(), "ratio": round(full.size() / sk.size(), 3),
        "expand_device_ms": round(e, 3), "expand_device_ms_all": [round(v, 3) for v in expand_ms],
        "expand_device_GBps_out": round(full.size() / e / 1e6, 1),
        "create_full_ms": round(f, 1), "create_full_ms_all": [round(v, 1) for v in full_ms],
        "create_seeded_ms": round(s, 1), "create_seeded_ms_all": [round(v, 1) for v in seeded_ms],
        "expand_share_of_create_seeded": round(e / s, 4),
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
