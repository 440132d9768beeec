"""The rasterizer's compositing stage against its float64 reference, as numbers: the worst err / bound per output array, case and
run of tests/test_gpu_raster_comp_f64.py (both forward forms, the ordered backward's rows behind each, the default mode's outputs,
tight lists, recolor) and the vacuity shares (the share of counted elements whose bound is at least |reference|).

    python tools/raster_comp_parity.py OUT.json        (needs the GPU; profiles/raster_comp_parity.json is its output)

Nothing in the tests reads the file."""
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(path):
    warnings.filterwarnings("ignore")
    from tests import test_gpu_raster_comp_f64 as G
    for c in G.GRID:
        G.test_eight_lane_forward_and_the_backward_behind_it(c)
    for c in G.WIDE:
        G.test_wide_forward_and_the_backward_behind_it(c)
    G.test_tight_lists()
    for c in G.RECOLOR:
        G.test_recolor_forward_and_backward(c)
    out = {name: {"worst_err_over_bound": G.WORST[name], "vacuity": G.VAC.get(name, {})} for name in G.WORST}
    worst = {}
    for rec in out.values():
        for k, v in rec["worst_err_over_bound"].items():
            a = " ".join(k.split()[:2]) if k.startswith("recolor") else k.split()[0]
            worst[a] = max(worst.get(a, 0.0), v)
    out["_worst_over_the_grid"] = worst
    out["_largest_vacuity_share"] = max(s for rec in out.values() if "vacuity" in rec for s in rec["vacuity"].values())
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({"cases": len(G.WORST), "worst": worst, "largest_vacuity_share": out["_largest_vacuity_share"]}))


if __name__ == "__main__":
    main(sys.argv[1])
