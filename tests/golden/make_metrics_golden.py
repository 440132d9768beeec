"""tests/golden/metrics_expected.json from the float64 restatement of the evaluation report (tests/metrics_ref.py) itself, on its
seeded cases: per case ``out`` (l1, psnr, ssim, ms_ssim), ``mse``, ``levels`` ((6, C, 2): [ssim mean, cs mean]; NaN as null),
``relu_inputs`` ((C, 5)) and ``dev32``: the largest absolute deviation of the same ops in float32 from the float64 values over
ssim, ms_ssim and every level mean — a measurement of what evaluating the cancelling ``E[x^2] - mu^2`` in float32 costs, from
which the GPU test takes its tolerance.

    python tests/golden/make_metrics_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import metrics_ref as MR  # noqa: E402


def _list(a):
    return [None if (isinstance(v, float) and v != v) else v for v in np.asarray(a, dtype=np.float64).ravel().tolist()]


def main():
    torch.set_num_threads(1)  # (the float32 sums of the deviation measurement in one fixed order)
    cases = {}
    for name, shape, pair, ms in MR.cases():
        x, y = MR.make_pair(shape, pair)
        r64 = MR.image_metrics(x, y, clamp=False, ms_ssim=ms)
        r32 = MR.image_metrics(x, y, clamp=False, ms_ssim=ms, dtype=torch.float32)
        dev = [np.nanmax(np.abs(r32["levels"] - r64["levels"])), abs(r32["out"][0, 2] - r64["out"][0, 2])]
        if ms:
            dev.append(abs(r32["out"][0, 3] - r64["out"][0, 3]))
        cases[name] = {"shape": list(shape), "pair": pair, "ms_ssim": ms, "out": _list(r64["out"][0]), "mse": float(r64["mse"][0]),
                       "levels": _list(r64["levels"][0]), "relu_inputs": _list(r64["relu_inputs"][0]), "dev32": float(max(dev))}
        print("%-24s dev32 %.3g  out %s" % (name, cases[name]["dev32"], r64["out"][0]))
    with open(os.path.join(HERE, "metrics_expected.json"), "w") as f:
        json.dump({"seed": MR.SEED, "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
