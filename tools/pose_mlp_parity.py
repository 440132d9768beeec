"""The PoseMLP kernels against their float64 references, as numbers: the worst err / bound per array, case and path of
tests/test_gpu_pose_mlp_f64.py (the grid, every one-launch case again one launch per layer, the sixteen draws), the vacuity shares
(the share of non-zero-reference elements whose bound is at least |reference|) and the measured error of the embedding's sinf / cosf
in ulp of the result.

    python tools/pose_mlp_parity.py OUT.json        (needs the GPU; profiles/pose_mlp_parity.json is its output)

Nothing in the tests reads the file."""
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(path):
    warnings.filterwarnings("ignore")
    from tests import test_gpu_pose_mlp_f64 as G
    for c in G.GRID:
        G.test_grid_against_float64(c)
    for c in G.ONE_LAUNCH:
        G.test_one_launch_cases_again_one_launch_per_layer(c)
    for seed in range(len(G.DRAWS)):
        G.test_random_draws_against_float64(seed)
    G.test_measured_sincos_error_is_within_the_allowance()
    out = {name: {"worst_err_over_bound": G.WORST[name], "vacuity": G.VAC.get(name, {})} for name in G.WORST}
    worst = {}
    for rec in out.values():
        for k, v in rec["worst_err_over_bound"].items():
            worst[k] = max(worst.get(k, 0.0), v)
    out["_worst_over_the_grid"] = worst
    out["_largest_vacuity_share"] = max(s for rec in out.values() if "vacuity" in rec for s in rec["vacuity"].values())
    out["_sincos_worst_error_ulp"] = G.MEASURED["sincos_ulp"]
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({"cases": len(G.WORST), "worst": worst, "largest_vacuity_share": out["_largest_vacuity_share"],
                      "sincos_worst_error_ulp": G.MEASURED["sincos_ulp"]}))


if __name__ == "__main__":
    main(sys.argv[1])
