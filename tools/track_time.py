"""Time riggs_amd.track (one launch of csrc/track.hip per call) against the SAME filters written in torch ops on the device:
the smoother as unfold over the padded track, an einsum for the 4 x 4 moment matrices and torch.linalg.eigh; the one-euro filter as
a Python loop over the frames.  Sizes: smooth_track at (T, J, R) = (200, 24, 6), (200, 256, 15), (2000, 24, 15), batches B = 1 and
B = 60; one_euro_track at T = 200 and at T = 1 (OneEuroTrack.filter: the streaming case), J = 24 and 256.  The two forms' results are
compared first.  Device events around repeated calls, after a warm-up; milliseconds per call.  Needs the GPU.
Writes profiles/track_times.json (or the path after --out)."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from riggs_amd import track as TR  # noqa: E402
from pose_solve_common import timed  # noqa: E402  (tools/ is the script's directory)


def make_track(B, T, J, seed, dev):
    """A random walk of 0.15 rad per frame per joint with 0.3 rad of noise, random signs and scales, confidences with 20 % gaps."""
    g = torch.Generator().manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(B, 1, J, 4, generator=g), dim=-1).repeat(1, T, 1, 1)
    q = torch.nn.functional.normalize(q + torch.cumsum(0.075 * torch.randn(B, T, J, 4, generator=g), 1) * 0.3 + 0.15 * torch.randn(B, T, J, 4, generator=g), dim=-1)
    q = q * (torch.randint(0, 2, (B, T, J, 1), generator=g) * 2 - 1) * (0.5 + 1.5 * torch.rand(B, T, J, 1, generator=g))
    w = 0.1 + 0.9 * torch.rand(B, T, J, generator=g)
    w[torch.rand(B, T, J, generator=g) < 0.2] = 0
    trans = torch.cumsum(0.05 * torch.randn(B, T, 3, generator=g), 1)
    return q.to(dev).contiguous(), trans.to(dev).contiguous(), w.to(dev).contiguous()


def torch_smooth(q, trans, w, taps):
    """The clipped window in torch ops: (B, T, J, 4), (B, T, 3), (B, T, J), taps (R + 1,) -> rotations, translations."""
    R = taps.shape[0] - 1
    k = torch.cat([taps.flip(0)[:-1], taps])                                   # (2R + 1,)
    qn = torch.nn.functional.normalize(q, dim=-1) * (w > 0)[..., None]
    pad = lambda a: torch.nn.functional.pad(a, (0, 0) * (a.dim() - 2) + (R, R))  # noqa: E731  (zeros outside the track)
    qw = pad(qn).unfold(1, 2 * R + 1, 1)                                       # (B, T, J, 4, 2R + 1)
    ww = pad(w.clamp_min(0)).unfold(1, 2 * R + 1, 1) * k                       # (B, T, J, 2R + 1)
    M = torch.einsum("ntjaw,ntjbw,ntjw->ntjab", qw, qw, ww)
    vec = torch.linalg.eigh(M)[1][..., 3]
    vec = vec * torch.where((vec * qn).sum(-1, keepdim=True) < 0, -1.0, 1.0)
    tw = pad(torch.ones_like(trans[..., 0])).unfold(1, 2 * R + 1, 1) * k       # (B, T, 2R + 1)
    tp = pad(trans).unfold(1, 2 * R + 1, 1)                                    # (B, T, 3, 2R + 1)
    return vec, (tp * tw[:, :, None]).sum(-1) / tw.sum(-1, keepdim=True)


def torch_one_euro(q, trans, rate, fmin, beta, fd):
    """All samples valid: (B, T, J, 4), (B, T, 3) -> the filtered rotations (B, T, J, 4); a Python loop over the frames."""
    alpha = lambda f, dt: 1.0 / (1.0 + 1.0 / (2.0 * math.pi * f * dt))  # noqa: E731
    dt = 1.0 / rate
    x = torch.nn.functional.normalize(q, dim=-1)
    f, om, out = x[:, 0], torch.zeros_like(x[:, 0, :, 0]), [x[:, 0]]
    for t in range(1, q.shape[1]):
        dot = (x[:, t] * f).sum(-1)
        v = torch.where(dot[..., None] < 0, -x[:, t], x[:, t])
        th = torch.acos(dot.abs().clamp(max=1.0))
        om = alpha(fd, dt) * (2.0 * th / dt) + (1.0 - alpha(fd, dt)) * om
        al = alpha(fmin + beta * om, dt)
        sn = torch.sin(th)
        lin = sn <= 1e-6
        w0 = torch.where(lin, 1.0 - al, torch.sin((1.0 - al) * th) / sn)
        w1 = torch.where(lin, al, torch.sin(al * th) / sn)
        f = torch.nn.functional.normalize(w0[..., None] * f + w1[..., None] * v, dim=-1)
        out.append(f)
    return torch.stack(out, 1)


def angle(a, b):
    """The largest angle between two sets of rotations, 2 acos |dot|, from the chord (acos loses half its digits next to 1)."""
    a, b = torch.nn.functional.normalize(a.double(), dim=-1), torch.nn.functional.normalize(b.double(), dim=-1)
    chord = torch.minimum((a - b).norm(dim=-1), (a + b).norm(dim=-1))
    return float((4.0 * torch.asin((chord / 2.0).clamp(max=1.0))).max())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_times.json"))
    ap.add_argument("--reps", type=int, default=200, help="timed calls of the library (the torch-op forms take a tenth)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "track_time.py measures on the GPU"
    dev = torch.device("cuda")
    rows = []
    for T, J, R in ((200, 24, 6), (200, 256, 15), (2000, 24, 15)):
        for B in (1, 60):
            q, trans, w = make_track(B, T, J, 100 + J + T, dev)
            sigma = R / 3.0
            track = {"local_rotation": q, "global_trans": trans}
            taps = torch.tensor(TR.gaussian_taps(sigma, R)[1], dtype=torch.float64).float().to(dev)
            out = TR.smooth_track(track, sigma, radius=R, weights=w)
            tq, tt = torch_smooth(q, trans, w, taps)
            held = out["support"] > 0
            row = {"filter": "smooth_track", "T": T, "J": J, "R": R, "B": B, "max_angle_diff_rad": angle(out["local_rotation"][held], tq[held]),
                   "max_abs_diff_trans": float((out["global_trans"] - tt).abs().max()),
                   "track_ms": timed(lambda: TR.smooth_track(track, sigma, radius=R, weights=w), args.reps),
                   "torch_ops_ms": timed(lambda: torch_smooth(q, trans, w, taps), max(3, args.reps // 10))}
            row["speedup"] = row["torch_ops_ms"] / row["track_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    euro = dict(rate=30.0, min_cutoff=1.5, beta=0.4, d_cutoff=1.0)
    for J in (24, 256):
        for B in (1, 60):
            q, trans, _ = make_track(B, 200, J, 300 + J, dev)
            track = {"local_rotation": q, "global_trans": trans}
            out = TR.one_euro_track(track, **euro)
            tq = torch_one_euro(q, trans, euro["rate"], euro["min_cutoff"], euro["beta"], euro["d_cutoff"])
            row = {"filter": "one_euro_track", "T": 200, "J": J, "B": B, "max_angle_diff_rad": angle(out["local_rotation"], tq),
                   "track_ms": timed(lambda: TR.one_euro_track(track, **euro), args.reps),
                   "torch_ops_ms": timed(lambda: torch_one_euro(q, trans, euro["rate"], euro["min_cutoff"], euro["beta"], euro["d_cutoff"]),
                                         max(3, args.reps // 40))}
            row["speedup"] = row["torch_ops_ms"] / row["track_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
        # the streaming case: one frame per launch, the state on the device; the torch-op form is one step of the loop above
        q, trans, _ = make_track(1, 2, J, 500 + J, dev)
        f = TR.OneEuroTrack(J, **euro)
        pose = {"local_rotation": q[0, 1], "global_trans": trans[0, 1:2]}
        f.filter({"local_rotation": q[0, 0], "global_trans": trans[0, :1]})
        row = {"filter": "OneEuroTrack.filter", "T": 1, "J": J, "B": 1, "track_ms": timed(lambda: f.filter(pose), args.reps),
               "torch_ops_ms": timed(lambda: torch_one_euro(q, trans, euro["rate"], euro["min_cutoff"], euro["beta"], euro["d_cutoff"]), args.reps)}
        row["speedup"] = row["torch_ops_ms"] / row["track_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        json.dump({"device": torch.cuda.get_device_name(0), "what": "ms per call, device events around repeated calls after a warm-up; track = one "
                   "launch of csrc/track.hip (plus torch's allocations), torch_ops = the same filter in torch ops on the device (smoother: "
                   "unfold, einsum, torch.linalg.eigh; one-euro: a Python loop over the frames)", "rows": rows}, f_, indent=1)


if __name__ == "__main__":
    main()
