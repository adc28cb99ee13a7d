"""One host-buffer board through the two ways a C caller can get its digest, in one process:

  split    omr_detect_batch, then omr_encode_indices per index ciphertext, then omr_encode_payloads
           (the pertinency vector crosses the boundary: D x 32 KiB down, then up once per call)
  session  omr_digest_begin, one omr_digest_update, omr_digest_read

    python tools/digest_session_bench.py [-D 16384] [--repeat 2] [--out FILE.json]

Per flow: wall time, the device memory in use before / at the peak / after (hipMemGetInfo through
torch.cuda.mem_get_info, polled from a thread while the flow runs; the library calls release the
GIL) and the host bytes the flow needs for the pertinency vector. Checks that both digests are
equal and prints one JSON line. DESIGN.md section 8 records a run.
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-omr_amd"))
import torch  # noqa: E402  (before libomr_gpu.so: one HIP runtime per process, see tests/conftest.py)

import omr_amd as A  # noqa: E402


class PeakUse:
    """Device bytes in use (total - free), polled every few milliseconds."""

    def __enter__(self):
        self.before = self.peak = self.used()
        self._stop = threading.Event()
        self._t = threading.Thread(target=self._poll, daemon=True)
        self._t.start()
        return self

    @staticmethod
    def used():
        free, total = torch.cuda.mem_get_info(0)
        return total - free

    def _poll(self):
        while not self._stop.wait(0.003):
            self.peak = max(self.peak, self.used())

    def __exit__(self, *exc):
        self._stop.set()
        self._t.join()
        self.after = self.used()
        self.peak = max(self.peak, self.after)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-D", type=int, default=16384)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    D = args.D
    torch.cuda.init()
    sk, other = A.SecretKeyPack(42), A.SecretKeyPack(4242)
    dk = sk.generate_detection_key(7)
    # a few distinct clues tiled over the board (the time does not depend on their values); message 0
    # and every 1024th are pertinent
    base = min(D, 1024)
    ca, cb = other.gen_clues(2, 0, base)
    pa, pb = sk.gen_clues(1, 0, 1)
    ca[0], cb[0] = pa[0], pb[0]
    reps = (D + base - 1) // base
    ca, cb = np.tile(ca, (reps, 1))[:D].copy(), np.tile(cb, (reps, 1))[:D].copy()
    payloads = np.random.default_rng(3).integers(0, 256, (D, A.PAYLOAD_LENGTH)).astype(np.uint16)
    rp = A.RetrievalParams(D, reps)
    wseed = bytes(range(32))
    weights = A.payload_weights(wseed, rp)
    det = A.Detector(dk)
    det.detect_batch(ca[:128], cb[:128])  # warm-up of the throughput kernels

    def split():
        pv = det.detect_batch(ca, cb)
        idx = np.stack([det.encode_pertinent_indices(rp, pv, 9, c) for c in range(rp.max_encode_indices_cipher_count)])
        return idx, det.encode_pertinent_payloads(pv, payloads, weights, rp)

    def session():
        with det.digest_session(D, reps, 9, wseed) as dg:
            dg.update(ca, cb, payloads, 0)
            res = dg.read()
            session.info = dg.info()
        return res

    out = {"D": D, "index_ct": rp.max_encode_indices_cipher_count, "payload_ct": rp.cmb_cipher_count, "runs": []}
    digests = {}
    for r in range(args.repeat):
        for name, fn in (("split", split), ("session", session)):
            with PeakUse() as m:
                t = time.perf_counter()
                digests[name] = fn()
                wall = time.perf_counter() - t
            out["runs"].append({"flow": name, "run": r, "wall_s": round(wall, 4),
                                "device_before_MiB": m.before >> 20, "device_peak_MiB": m.peak >> 20,
                                "device_after_MiB": m.after >> 20,
                                "device_peak_delta_MiB": (m.peak - m.before) >> 20,
                                "host_pv_MiB": (D * 32768 >> 20) if name == "split" else 0})
    out["pv_capacity_messages"] = session.info["pv_capacity_messages"]
    out["digests_equal"] = bool(np.array_equal(digests["split"][0], digests["session"][0]) and
                                np.array_equal(digests["split"][1], digests["session"][1]))
    det.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if out["digests_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
