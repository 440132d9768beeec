"""The image loss and the evaluation report against their float64 references, as numbers: the worst err / bound per array and case of
tests/test_gpu_ssim_window_f64.py (the loss grid, the backward's options, the metrics cases), the vacuity shares (the share of
non-zero-reference elements whose bound reaches |reference|), the worst bound / (k magnitude) of the structural families, and —
computed on the host from the float32 restatement — every planted fault against the bars of tests/test_gpu_loss.py and
tests/test_gpu_metrics.py on the same input.

    python tools/ssim_window_parity.py OUT.json        (needs the GPU; profiles/ssim_window_parity.json is its output)

Nothing in the tests reads the file."""
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fault_table():
    from tests import ssim_window_ref as S
    rows = {}
    for fault in list(S.LOSS_FAULTS) + ["window_f64_for_f32"]:
        if fault in S.LOSS_FAULTS:
            case, _ = S.fault_case(fault)
            x, y, state, out3, dx = S.restate_case(case, fault=fault)
        else:
            case, _ = S.fault_case("h_tap_0")
            x, y, state, out3, dx = S.restate_case(case, win=S.win_f64())
        res = S.check_loss(case, x, y, state, out3, dx)
        rows[fault] = {"rejected_on": S.bad_arrays(res), "old_bars_reject": S.old_bars_loss(x, y, out3, dx, case["g"]),
                       "worst_err_over_bound": max([v["worst"] for v in res.values() if isinstance(v, dict)])}
    for fault, (name, _) in S.METRICS_FAULTS.items():
        _, shape, family, ms = next(c for c in S.METRICS_CASES if c[0] == name)
        x, y = S.metrics_inputs(shape, family)
        got = S.restate_metrics(x, y, False, ms, fault=fault)
        res = S.check_metrics(x, y, False, ms, got)
        rows[fault] = {"rejected_on": S.bad_arrays(res), "old_bars_reject": S.old_bars_metrics(x, y, ms, got),
                       "worst_err_over_bound": max([v["worst"] for v in res.values() if isinstance(v, dict)])}
    return rows


def main(path):
    warnings.filterwarnings("ignore")
    from tests import test_gpu_ssim_window_f64 as G
    for c in G.GRID:
        G.test_loss_grid_against_float64(c)
    for shape, family in G.OPTION_SHAPES:
        G.test_backward_options_one_by_one(shape, family)
    for name, shape, family, ms in G.S.METRICS_CASES:
        G.test_metrics_pools_partials_and_means(name, shape, family, ms)
    for shape, ms in (((1, 75, 43), False), ((3, 161, 161), True), ((1, 385, 385), True)):
        G.test_metrics_clamp_on_load_equals_clamped_inputs_in_every_partial(shape, ms)
    out = {name: {"worst_err_over_bound": G.WORST[name], "vacuity": G.VAC[name]} for name in G.WORST}
    worst, smallest = {}, {}
    for rec in out.values():
        for k, v in rec["worst_err_over_bound"].items():
            worst[k] = max(worst.get(k, 0.0), v)
    for k in worst:  # the smallest worst-case ratio of an array over the cases where it is not exact
        vals = [rec["worst_err_over_bound"][k] for rec in out.values() if rec["worst_err_over_bound"].get(k, 0.0) > 0.0]
        smallest[k] = min(vals) if vals else 0.0
    scored = [n for n in out if not any(f in n for f in G.S.STRUCTURAL)]
    summary = {"_worst_over_the_cases": worst, "_smallest_worst_ratio_per_array": smallest,
               "_arrays_whose_worst_ratio_is_below_0.01": sorted(k for k, v in worst.items() if 0.0 < v < 0.01),
               "_largest_vacuity_share": max(s for n in scored for s in out[n]["vacuity"].values()),
               "_structural_worst_bound_over_k_magnitude": max(G.STRUCT.values()), "_planted_faults": fault_table()}
    out.update(summary)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({k: v for k, v in summary.items() if k != "_planted_faults"} | {"cases": len(G.WORST)}))


if __name__ == "__main__":
    main(sys.argv[1])
