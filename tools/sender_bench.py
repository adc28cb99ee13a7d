"""The sender (include/omr_gpu.h, "Sender") measured against what it replaces.

    python tools/sender_bench.py [--d 65536] [--open-d 1048576] [--parent-lib PATH] [--out profiles/sender/time.json]

mixed    a two-recipient board of D messages: one omr_sender_gen_clues_device against the parent's way, two
         omr_gen_clues_device calls and the masked merge of bench.py.
one_key  the sender over one key against omr_gen_clues_device: the same clues, the sender's kernel fetching
         its key from the table and its tables uploaded once instead of per call.
gather   n_keys in {1, 2, 1,024, 65,536} (a 128 MiB table) with uniformly random recipients: time per clue
         and the rate of the clue stores against the HBM peak.
open     omr_clue_open_device against omr_clue_open on 16 host threads over --open-d messages, and the rate
         of the kernel's clue read against the HBM peak.
--parent-lib names a libomr_gpu.so built from the parent commit for the two omr_gen_clues_device baselines;
without it they run from this build, whose gen_clues_kernel and entry point are the parent's, unchanged.

Device events around each call on one stream (every call returns after the stream has finished its work),
after a warm-up, the versions of a comparison alternating inside one process; each figure is the median of
REPEAT with its own max / min next to it. Prints one JSON line and writes it to --out.
"""
import argparse
import ctypes as C
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

REPEAT, WARMUP = 7, 2
HBM_PEAK = 8.0e12  # bytes/s
CLUE_BYTES = (A.N0 + A.CLUE_COUNT) * 2


def event_ms(call):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    call()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def alternate(calls):
    """name -> times (ms) of REPEAT rounds, the calls of a round taken in turn, after WARMUP rounds."""
    for _ in range(WARMUP):
        for c in calls.values():
            c()
    times = {k: [] for k in calls}
    for _ in range(REPEAT):
        for k, c in calls.items():
            times[k].append(event_ms(c))
    return times


def figure(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "max_over_min": round(max(ms) / min(ms), 3)}


class Parent:
    """omr_gen_clues_device of a pack, from --parent-lib when given (its own pack: handles are not shared
    between two libraries), else from this build."""

    def __init__(self, path, seed):
        self.external = bool(path)
        if path:
            L = C.CDLL(path)
            L.omr_keygen_secret.argtypes = [C.c_uint64, C.POINTER(C.c_void_p)]
            L.omr_gen_clues_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_size_t, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
            self.h = C.c_void_p()
            assert L.omr_keygen_secret(seed, C.byref(self.h)) == 0
            self.L = L
        else:
            self.pack = A.SecretKeyPack(seed)

    def gen(self, seed, first, count, da, db):
        if self.external:
            assert self.L.omr_gen_clues_device(self.h, seed, first, count, da, db, None) == 0
        else:
            self.pack.gen_clues_device(seed, first, count, da, db)


def clue_buffers(D):
    return (torch.empty((D, A.N0), dtype=torch.int16, device="cuda:0"),
            torch.empty((D, A.CLUE_COUNT), dtype=torch.int16, device="cuda:0"))


def mixed_and_one_key(D, parent_lib):
    pa, pb = A.SecretKeyPack(42), A.SecretKeyPack(4242)
    qa, qb = Parent(parent_lib, 42), Parent(parent_lib, 4242)
    mask = np.random.default_rng(2025).random(D) < 0.5
    d_mask = torch.from_numpy(mask).to("cuda:0")[:, None]
    d_rec = torch.from_numpy(np.where(mask, 0, 1).astype(np.int32)).to("cuda:0")
    two = A.Sender([pa.clue_key(), pb.clue_key()], device=0)
    one = A.Sender(pa.clue_key(), device=0)
    xa, xb = clue_buffers(D)
    ya, yb = clue_buffers(D)
    sa, sb = clue_buffers(D)
    merged = {}

    def parent_mixed():
        qa.gen(1000, 0, D, xa.data_ptr(), xb.data_ptr())
        qb.gen(1000, 0, D, ya.data_ptr(), yb.data_ptr())
        merged["a"] = torch.where(d_mask, xa, ya).contiguous()
        merged["b"] = torch.where(d_mask, xb, yb).contiguous()

    t = alternate({"parent": parent_mixed,
                   "sender": lambda: two.gen_clues_device(1000, 0, D, sa.data_ptr(), sb.data_ptr(), d_rec.data_ptr())})
    assert torch.equal(merged["a"], sa) and torch.equal(merged["b"], sb), "the two boards differ"
    mixed = {"messages": D, "recipients": 2, "parent_two_generations_and_merge": figure(t["parent"]),
             "sender_one_launch": figure(t["sender"]), "same_bits": True,
             "sender_over_parent": round(statistics.median(t["sender"]) / statistics.median(t["parent"]), 3)}

    t = alternate({"parent": lambda: qa.gen(1000, 0, D, xa.data_ptr(), xb.data_ptr()),
                   "sender": lambda: one.gen_clues_device(1000, 0, D, sa.data_ptr(), sb.data_ptr())})
    assert torch.equal(xa, sa) and torch.equal(xb, sb), "one key: the clues differ"
    p, s = figure(t["parent"]), figure(t["sender"])
    one_key = {"messages": D, "parent_gen_clues_device": p, "sender": s, "same_bits": True,
               "sender_over_parent": round(s["median_ms"] / p["median_ms"], 3),
               "condition": "sender median <= parent median x parent max/min",
               "condition_met": bool(s["median_ms"] <= p["median_ms"] * p["max_over_min"])}
    two.close()
    one.close()
    return mixed, one_key


def gather(D):
    rng = np.random.default_rng(7)
    da, db = clue_buffers(D)
    rows = []
    for n_keys in (1, 2, 1024, 65536):
        table = rng.integers(0, 2048, (n_keys, 2, A.N0), dtype=np.uint16)
        snd = A.Sender(table, device=0)
        d_rec = torch.from_numpy(rng.integers(0, n_keys, D).astype(np.int32)).to("cuda:0")
        t = alternate({"sender": lambda: snd.gen_clues_device(5, 0, D, da.data_ptr(), db.data_ptr(), d_rec.data_ptr())})
        f = figure(t["sender"])
        sec = f["median_ms"] * 1e-3
        f.update({"n_keys": n_keys, "table_bytes": int(table.nbytes), "ns_per_clue": round(sec / D * 1e9, 2),
                  "store_bytes_per_s": round(D * CLUE_BYTES / sec, 1),
                  "store_share_of_hbm_peak": round(D * CLUE_BYTES / sec / HBM_PEAK, 5),
                  "key_fetch_bytes_per_s": round(D * 2048 / sec, 1)})
        rows.append(f)
        snd.close()
        del d_rec
    return {"messages": D, "hbm_peak_bytes_per_s": HBM_PEAK, "per_table": rows}


def opening(D):
    packs = [A.SecretKeyPack(s) for s in (42, 4242, 424242)]
    snd = A.Sender([p.clue_key() for p in packs], device=0)
    rec = np.random.default_rng(9).integers(0, 3, D).astype(np.int32)
    d_rec = torch.from_numpy(rec).to("cuda:0")
    da, db = clue_buffers(D)
    snd.gen_clues_device(77, 0, D, da.data_ptr(), db.data_ptr(), d_rec.data_ptr())
    snd.close()
    d_val = torch.empty((D, A.CLUE_COUNT), dtype=torch.uint8, device="cuda:0")
    d_pert = torch.empty(D, dtype=torch.uint8, device="cuda:0")
    d_noise = torch.empty(D, dtype=torch.uint8, device="cuda:0")
    t = alternate({"device": lambda: packs[0].open_clues_device(da.data_ptr(), db.data_ptr(), D, d_val.data_ptr(),
                                                                d_pert.data_ptr(), d_noise.data_ptr())})
    ca = da.cpu().numpy().view(np.uint16)
    cb = db.cpu().numpy().view(np.uint16)
    cpu = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = packs[0].open_clues(ca, cb, nthreads=16)
        cpu.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(d_pert.cpu().numpy(), want["pertinent"]) and np.array_equal(want["pertinent"], rec == 0)
    assert np.array_equal(d_val.cpu().numpy(), want["values"]) and np.array_equal(d_noise.cpu().numpy(), want["max_abs_noise"])
    f = figure(t["device"])
    sec = f["median_ms"] * 1e-3
    read = D * CLUE_BYTES
    return {"messages": D, "device": f, "cpu_16_threads": figure(cpu), "same_results": True,
            "cpu_over_device": round(statistics.median(cpu) / f["median_ms"], 1),
            "clue_read_bytes_per_s": round(read / sec, 1), "read_share_of_hbm_peak": round(read / sec / HBM_PEAK, 4),
            "hbm_peak_bytes_per_s": HBM_PEAK, "note": "the device time is the whole call: launch, kernel and the "
            "stream synchronise it returns after"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=65536)
    ap.add_argument("--open-d", type=int, default=1 << 20)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sender", "time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sender_bench: no GPU; nothing is measured on the CPU")
    torch.cuda.init()
    mixed, one_key = mixed_and_one_key(args.d, args.parent_lib)
    res = {"device": torch.cuda.get_device_name(0), "repeat": REPEAT, "warmup": WARMUP,
           "baseline_library": "built from the parent commit" if args.parent_lib else "this build (gen_clues_kernel unchanged)",
           "mixed": mixed, "one_key": one_key, "gather": gather(args.d), "open": opening(args.open_d)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
