"""Per-node medians over the replayed steps of a rocprofv3 kernel trace (rocpd database), as JSON on stdout.
usage: python tools/timeline_medians.py <results.db> [anchor-kernel-substring] [steps-to-drop]
  rocprofv3 --kernel-trace -f rocpd -d out -o t -- python bench.py --steps 60 --warmup 5
A step is what lies between two launches of the anchor kernel (tools/timeline.py prints the fastest one); the steps with the
usual number of kernels are kept, the first `steps-to-drop` of them (default 5) dropped."""
import json
import sqlite3
import statistics
import sys
from collections import Counter


def medians(db_path, anchor="pm_forward_fused", drop=5):
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, start, end from kernels order by start").fetchall()
    idx = [i for i, r in enumerate(rows) if anchor in r[0]]
    steps = [rows[a:b] for a, b in zip(idx[:-1], idx[1:])]
    if not steps:
        return {}
    n = Counter(len(s) for s in steps).most_common(1)[0][0]
    steps = [s for s in steps if len(s) == n][int(drop):]
    out = {"steps": len(steps), "nodes_us": {}}
    for k in range(n):
        d = [(s[k][2] - s[k][1]) / 1e3 for s in steps]
        name = "%02d %s" % (k, steps[0][k][0].split("(")[0].replace("riggs::", "").replace("void ", ""))
        out["nodes_us"][name] = {"median": round(statistics.median(d), 2), "stdev": round(statistics.pstdev(d), 2)}
    period = [(b[0][1] - a[0][1]) / 1e3 for a, b in zip(steps[:-1], steps[1:])]
    out["step_period_us_median"] = round(statistics.median(period), 1) if period else None
    out["sum_of_node_medians_us"] = round(sum(v["median"] for v in out["nodes_us"].values()), 2)
    return out


if __name__ == "__main__":
    print(json.dumps(medians(*sys.argv[1:]), indent=1))
