"""Stage-1 playback at the scale its users run: ``ControlNodeWarp.deform_sequence`` (one network call + one blend launch for a
track) against the per-frame loop of ``ControlNodeWarp.forward``, in the same process, on the same inputs, under ``no_grad``.

    python tools/cnode_sequence_time.py [--out profiles/cnode_sequence_times.json] [--reps 15]

Every figure is a median over ``reps`` repetitions of device-event times after warm-up, the two versions alternating inside a
repetition.  "module": the whole call, node network (DeformNetwork) included.  "blend": the blend launches alone on given node
attributes — ``control_node_blend_sequence`` against T calls of ``control_node_blend`` — which is where the store roofline is
taken: the sequence kernel must write 40 B per Gaussian and frame (d_xyz, d_rotation, d_scaling), over the 8 TB/s peak of HBM3E.
Needs the GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from riggs_amd import control_nodes as CN  # noqa: E402
from riggs_amd.node_network import DeformNetwork  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, the spec figure
STORE_BYTES = 40   # per Gaussian and frame


def stage(N, M, hyper, local_frame, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(N, 3, generator=g) - 0.5).cuda()
    torch.manual_seed(seed)
    cn = CN.ControlNodeWarp(node_num=M, K=3, hyper_dim=hyper, local_frame=local_frame,
                            network=DeformNetwork(is_blender=True, local_frame=local_frame)).cuda().eval()
    with torch.no_grad():
        cn.nodes.copy_(torch.cat([x[torch.randperm(N, generator=g)[:M].cuda()], 1e-2 + 0.02 * torch.randn(M, hyper, generator=g).cuda()], -1))
        cn._node_radius.fill_(-2.0)
    feature = torch.cat([0.02 * torch.randn(N, hyper, generator=g), 2.0 + torch.randn(N, 1, generator=g)], -1).cuda()
    return cn, x, feature, torch.sigmoid(feature[:, -1:])


def medians(fns, reps, warmup=3):
    """Median milliseconds of each callable; they alternate inside a repetition."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [statistics.median(t) for t in times]


def track(cn, x, feature, mask, T, chunk, reps):
    """ms per frame of the loop and of the sequence (in chunks of ``chunk`` frames), module level and blend level."""
    times = torch.linspace(0, 1, T, device="cuda")
    N, M = x.shape[0], cn.node_num

    def loop():
        for f in range(T):
            cn(x, times[f], feature, mask)

    def seq():
        for c0 in range(0, T, chunk):
            cn.deform_sequence(x, times[c0:c0 + chunk], feature, mask)

    with torch.no_grad():
        nd = cn.node_deform(t=times[None, :, None].expand(M, T, 1))
        attrs = {k: v.transpose(0, 1).contiguous() for k, v in nd.items() if v is not None and k != "hidden"}
        per = [{k: v[f] for k, v in attrs.items()} for f in range(T)]
        nw = cn._node_weight if cn.with_node_weight else None
        cfg = dict(K=cn.K, hyper_dim=cn.hyper_dim, local_frame=cn.local_frame, d_rot_as_res=cn.d_rot_as_res)

        def blend_loop():
            for f in range(T):
                CN.control_node_blend(x, feature, mask, cn.nodes, cn._node_radius, nw, per[f], **cfg)

        def blend_seq():
            for c0 in range(0, T, chunk):
                CN.control_node_blend_sequence(x, feature, mask, cn.nodes, cn._node_radius, nw,
                                               {k: v[c0:c0 + chunk] for k, v in attrs.items()}, **cfg)

        # the results must not differ: the same lists, outputs to float32 rounding
        a = cn.deform_sequence(x, times[:min(T, chunk)], feature, mask)
        b = cn(x, times[0], feature, mask)
        assert torch.equal(a["nn_idx"], b["nn_idx"])
        diff = max(float((a[k][0] - b[k]).abs().max()) for k in ("d_xyz", "d_rotation", "d_scaling"))
        assert diff <= 1e-5, diff
        m_loop, m_seq = medians([loop, seq], reps)
        b_loop, b_seq = medians([blend_loop, blend_seq], reps)
    roof_ms = STORE_BYTES * N * T / HBM_PEAK * 1e3
    return {"N": N, "M": M, "T": T, "chunk": chunk,
            "module_loop_ms_per_frame": m_loop / T, "module_sequence_ms_per_frame": m_seq / T, "module_ratio_loop_over_sequence": m_loop / m_seq,
            "blend_loop_ms_per_frame": b_loop / T, "blend_sequence_ms_per_frame": b_seq / T, "blend_ratio_loop_over_sequence": b_loop / b_seq,
            "store_roofline_ms_per_frame": roof_ms / T, "blend_sequence_fraction_of_store_roofline": roof_ms / b_seq,
            "max_abs_difference_frame0": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "cnode_sequence_times.json"))
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cnode_sequence_time: needs the GPU (nothing is measured without it)")
    res = {"machine": torch.cuda.get_device_name(0), "torch": torch.__version__, "reps": args.reps,
           "method": "medians of device-event times after 3 warm-up rounds; loop and sequence alternate inside a repetition; no_grad",
           "pass_frames": CN.sequence_pass_frames(512, 3), "shipped_shape": [], "default_node_count": []}
    cn, x, feature, mask = stage(300_000, 512, 8, True, 1)
    for T in (1, 8, 32, 150):
        res["shipped_shape"].append(track(cn, x, feature, mask, T, T, max(5, args.reps // (1 + T // 50))))
        print(json.dumps(res["shipped_shape"][-1]), flush=True)
    del cn, x, feature, mask
    torch.cuda.empty_cache()
    cn, x, feature, mask = stage(100_000, 1024, 8, False, 2)
    res["default_node_count"].append(track(cn, x, feature, mask, 200, 32, max(5, args.reps // 3)))
    print(json.dumps(res["default_node_count"][-1]), flush=True)
    for r in res["shipped_shape"] + res["default_node_count"]:
        if r["T"] >= 8:
            assert r["module_sequence_ms_per_frame"] < r["module_loop_ms_per_frame"], r
            assert r["blend_sequence_ms_per_frame"] < r["blend_loop_ms_per_frame"], r
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", os.path.abspath(args.out))


if __name__ == "__main__":
    main()
