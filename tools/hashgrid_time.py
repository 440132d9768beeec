"""Times the hash-grid encoding (riggs_amd.hash_network.HashGridEncoding: csrc/hashgrid.hip) on the reference configuration
(12 levels, 2 features, 2^19 entries, base 16, scale 2.0): the forward alone, and the forward plus the table-gradient backward
(the ``zeros`` of the 40 MB gradient table inside the timed region), at D = 3 and D = 4 and at R = 512 rows (a node query) and
R = 65 536 rows (the node-Gaussian stage).  Beside each, a torch-op form of the same arithmetic on the same GPU: one index tensor
(R, L, 2^D) and one weight tensor from elementwise ops, one gather, a weighted sum; backward: ``zeros_like`` + one ``index_add_``.
Device time by events around ``inner`` back-to-back calls, the median of ``--repeats`` windows, the two forms alternating; the
outputs of the two forms are compared first.  Writes profiles/hashgrid_times.json (or the path after --out)."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from riggs_amd.hash_network import HashGridEncoding  # noqa: E402

PRIMES = (1, 2654435761, 805459861, 3674653429)
M32 = 0xFFFFFFFF


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def torch_corners(x, levels):
    """(idx (R, L, 2^D) int64 into the whole table, w (R, L, 2^D) float32) with torch ops; uint32 arithmetic in int64 under a mask."""
    R, D = x.shape
    idx_l, w_l = [], []
    for scale, res, size, off, hashed in levels:
        pos = (x.double() * scale + 0.5).float()     # = fmaf(scale, x, 0.5f): the product is exact in double, one rounding
        fl = torch.floor(pos)
        cell, frac = fl.to(torch.int64), pos - fl
        idx_k, w_k = [], []
        for k in range(1 << D):
            i, w, stride = None, None, 1
            for d in range(D):
                bit = (k >> d) & 1
                c = (cell[:, d] + bit) & M32
                wd = frac[:, d] if bit else 1.0 - frac[:, d]
                w = wd if w is None else w * wd
                term = (c * (PRIMES[d] if hashed else stride)) & M32
                i = term if i is None else ((i ^ term) if hashed else ((i + term) & M32))
                stride = (stride * res) & M32
            idx_k.append(i % size + off)
            w_k.append(w)
        idx_l.append(torch.stack(idx_k, -1))
        w_l.append(torch.stack(w_k, -1))
    return torch.stack(idx_l, 1), torch.stack(w_l, 1)


def torch_forward(x, table2, levels):
    idx, w = torch_corners(x, levels)
    return (table2[idx] * w[..., None]).sum(2).reshape(x.shape[0], -1), idx, w


def torch_forward_backward(x, table2, levels, g):
    out, idx, w = torch_forward(x, table2, levels)
    g_table = torch.zeros_like(table2)
    contrib = w[..., None] * g.view(x.shape[0], -1, 1, 2)
    g_table.index_add_(0, idx.reshape(-1), contrib.reshape(-1, 2))
    return out, g_table


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    repeats = arg("--repeats", 7)
    out = {"what": "grid encoding, reference configuration (L 12, F 2, 2^19, base 16, scale 2.0); device ms per call = median of "
                   "%d windows of `inner` back-to-back calls; hip = csrc/hashgrid.hip, torch = index tensors + gather + index_add_" % repeats,
           "device": torch.cuda.get_device_name(0), "cases": {}}
    g0 = torch.Generator().manual_seed(4)
    for D in (3, 4):
        enc = HashGridEncoding(D)
        with torch.no_grad():
            enc.params.uniform_(-1, 1)
        levels = enc.level_table()
        table2 = enc.params.detach().view(-1, 2)
        for R in (512, 65536):
            x = torch.rand(R, D, generator=g0).cuda()
            g = torch.randn(R, enc.n_output_dims, generator=g0).cuda()
            inner = 200 if R == 512 else 20

            def hip_fwd():
                with torch.no_grad():
                    return enc(x)

            def hip_fwd_bwd():
                enc.params.grad = None
                o = enc(x)
                o.backward(g)
                return o

            ref, ref_g = torch_forward_backward(x, table2, levels, g)
            got = hip_fwd_bwd()
            err = float((got.detach() - ref).abs().max())
            gerr = float((enc.params.grad.view(-1, 2) - ref_g).abs().max() / ref_g.abs().max())
            assert err < 1e-5 and gerr < 1e-4, (err, gerr)
            forms = {"hip_forward": hip_fwd, "torch_forward": lambda: torch_forward(x, table2, levels),
                     "hip_forward_backward": hip_fwd_bwd, "torch_forward_backward": lambda: torch_forward_backward(x, table2, levels, g)}
            for fn in forms.values():       # warm-up: code objects, the allocator
                window(fn, 3)
            runs = {k: [] for k in forms}
            for _ in range(repeats):        # the forms alternate inside every repeat
                for k, fn in forms.items():
                    runs[k].append(window(fn, inner))
            row = {"inner": inner, "forward_max_abs_diff": err, "table_grad_max_rel_diff": gerr}
            for k, v in runs.items():
                row[k + "_ms"] = statistics.median(v)
                row[k + "_min_max_ms"] = [min(v), max(v)]
            row["torch_over_hip_forward"] = row["torch_forward_ms"] / row["hip_forward_ms"]
            row["torch_over_hip_forward_backward"] = row["torch_forward_backward_ms"] / row["hip_forward_backward_ms"]
            out["cases"]["D%d_R%d" % (D, R)] = row
            print("D%d_R%d" % (D, R), json.dumps(row), flush=True)
        del enc, table2
    path = arg("--out", os.path.join(ROOT, "profiles", "hashgrid_times.json"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
