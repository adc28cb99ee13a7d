"""Rounding margins of the FFT kernels on crafted inputs (tests/acc_cases.py), measured: how close the
adversarial cases come to the a priori bound E of DESIGN.md §3a.

    python tools/crafted_acc_margin.py [--out profiles/crafted_acc/margins.json]

Per level (1: br1f and br1l guarded; 2: br2f guarded) and for the trace (trace_fft guarded), on bench.py's
key: each spectrally or sign-aligned case and a uniformly random accumulator through the same single CMUX
step (or one trace), one guarded launch each; the observed margin max |y - rint(y)| of that launch, the
a priori E and the key's kappa. Every output is compared with the oracle, and a breach (a guarded launch
that fell back to the exact NTT) or a margin above E exits non-zero. Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tfhe-omr_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (before libomr_gpu.so: one HIP runtime per process, see tests/conftest.py)

import acc_cases as AC  # noqa: E402
import oracle_lib as O  # noqa: E402
import omr_amd as A  # noqa: E402
import product_lib as PL  # noqa: E402
from fft_bound import apriori_bound_trace  # noqa: E402


def one(det, lvl, run, want):
    """The observed margin of level index lvl over one guarded launch, its output checked."""
    det.rounding_margin(reset=True)
    if not np.array_equal(run(), want):
        sys.exit("output differs from the oracle")
    return det.rounding_margin(reset=True)["observed"][lvl]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crafted_acc", "margins.json"))
    args = ap.parse_args()
    dk = PL.keys()[2]
    orc = O.OracleDetector(dk.bsk1, dk.ksk, dk.bsk2, dk.trace_key)
    det = A.Detector(dk)
    m = det.rounding_margin()
    res = {"key": {"pack": PL.SK_SEED, "seed": PL.KEY_SEED}}
    det.set_rounding_guard(True)
    for level in (1, 2):
        L = AC.LEVELS[level]
        cs = AC.cases(level, dk)
        cs["random"] = AC.random_case(L, dk)
        i, r, o, mstar, kappa = AC.spectral_peak(L, dk)
        entry = {"E": m["apriori"][level - 1], "kappa": m["kappa"][level - 1],
                 "peak": {"step": i, "row": r, "output": o, "point": mstar}}
        for path, thr in (("throughput", 0),) + ((("latency", 64),) if level == 1 else ()):
            det.set_latency_threshold(thr)
            obs = {}
            for name in AC.aligned_names(level) + ["random"]:
                lwe, acc0 = cs[name]
                if level == 1:
                    obs[name] = one(det, 0, lambda: det.blind_rotate_level1(lwe, acc0=acc0)[0], orc.br1_from(lwe, acc0))
                else:
                    obs[name] = one(det, 1, lambda: det.blind_rotate_level2(lwe, acc0=acc0)[0], orc.br2_from(lwe, acc0))
            entry[path] = obs
        res[f"level{level}"] = entry
    det.set_latency_threshold(0)
    ts = AC.trace_cases(dk)
    ts["random"] = AC.trace_random_case()
    i, r, o, mstar, kappa = AC.spectral_peak(AC.LT, dk)
    res["trace"] = {"E": apriori_bound_trace(dk), "kappa_first_step": kappa,
                    "peak": {"step": i, "row": r, "output": o, "point": mstar},
                    "throughput": {name: one(det, 1, lambda: det.trace(ts[name])[0], orc.trace(ts[name]))
                                   for name in AC.trace_aligned_names() + ["random"]}}
    res["breaches"] = det.exactness()["breaches"]
    det.close()
    worst = {k: max(max(v.values()) for p, v in res[k].items() if p in ("throughput", "latency"))
             for k in ("level1", "level2", "trace")}
    res["largest"] = {k: {"observed": worst[k], "E": res[k]["E"]} for k in worst}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if any(res["breaches"]) or any(v["observed"] > v["E"] for v in res["largest"].values()):
        sys.exit("a breach, or a margin above E")


if __name__ == "__main__":
    main()
