"""The per-Gaussian stage of the rasterizer against its float64 reference, as numbers: the worst err / bound per output array and
case of tests/test_gpu_raster_gauss_f64.py (forward state, and the backward in both launch forms of preprocess_bwd), and the
vacuity shares of tests/test_raster_gauss_ref_cpu.py (the share of counted elements whose bound is at least |reference|).

    python tools/raster_gauss_parity.py OUT.json        (needs the GPU; profiles/raster_gauss_parity.json is its output)

Nothing in the tests reads the file."""
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(path):
    warnings.filterwarnings("ignore")
    from tests import test_gpu_raster_gauss_f64 as G
    from tests import test_raster_gauss_ref_cpu as T
    out = {}
    for i, c in enumerate(G.GRID):
        tag = G.case_id(c)
        G.run_case(c)
        sh = T.vacuity(c)
        out["%02d-%s" % (i, tag)] = {"worst_err_over_bound": G.WORST[tag], "vacuity": {k: {"counted": n, "share": s} for k, (n, s) in sh.items()}}
    worst = {}
    for rec in out.values():
        for part in rec["worst_err_over_bound"].values():
            for k, v in part.items():
                worst[k] = max(worst.get(k, 0.0), v)
    out["_worst_over_the_grid"] = worst
    out["_largest_vacuity_share"] = max(v["share"] for rec in out.values() if "vacuity" in rec for v in rec["vacuity"].values())
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({"cases": len(G.GRID), "worst": worst, "largest_vacuity_share": out["_largest_vacuity_share"]}))


if __name__ == "__main__":
    main(sys.argv[1])
