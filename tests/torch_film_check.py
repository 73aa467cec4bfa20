"""Child process of test_gpu_film.py::test_torch_tensors_on_the_current_stream.

torch must own the process's HIP runtime before librtx loads,
so this runs in its own interpreter: torch first, then rtx. The film records
are a torch tensor made by torch work on a side stream, the context launches on
that stream (torch's current one), the results and segments are torch tensors
read back by torch, and a continuing call runs on the same tensors; afterwards
the context goes back to its own stream and traces again from host arrays.
argv[1]: a directory with queries.npy ((n, 16) float32), sums.npy ((n, 3)
float32), spheres.npy, mat_types.npy and mat_values.npy; argv[2] .. argv[5]:
the samples, the depth, img_w and img_h. Prints "ok" or raises."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytrace-we-gpu_amd"))
import rtx  # noqa: E402

d = sys.argv[1]
samples, depth, img_w, img_h = int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]), float(sys.argv[5])
queries = np.load(os.path.join(d, "queries.npy"))
sums = np.load(os.path.join(d, "sums.npy"))
n = len(queries)
assert queries.shape == (n, 16) and sums.shape == (n, 3) and samples > 2


def same(got, what):
    got = np.ascontiguousarray(got, np.float32).reshape(n, 4)[:, :3]
    if not ((got.view(np.uint32) == sums.view(np.uint32)) | (np.isnan(got) & np.isnan(sums))).all():
        raise SystemExit(f"{what}: sums differ")


torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
ctx = rtx.Context(0)
ctx.upload_world(rtx.World(np.load(os.path.join(d, "spheres.npy")), np.load(os.path.join(d, "mat_types.npy")),
                           np.load(os.path.join(d, "mat_values.npy")), depth, 1))
side = torch.cuda.Stream(device=dev)
host = torch.from_numpy(queries.copy())
seeds = {}
for order in ("given", "cost"):
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream != 0
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        # torch work on the stream, then the queries over its result, then torch work on the call's result
        t_q = (host.to(dev, non_blocking=True).view(torch.int32) + 0).view(torch.float32)
        t_r = torch.full((n, 4), -7, dtype=torch.int32, device=dev).view(torch.float32)
        t_s = torch.full((n,), -7, dtype=torch.int32, device=dev)
        got = ctx.trace_film(t_q, 2, img_w, img_h, order=order, results=t_r, segments=t_s)
        assert got[0] is t_r and got[1] is t_s and ctx.film_last_order() == "given"  # (2 samples: no more than the probe)
        first = t_s.clone()
        got = ctx.trace_film(t_q, samples - 2, img_w, img_h, order=order, results=t_r, segments=t_s, cont=True)
        assert got[0] is t_r and got[1] is t_s and ctx.film_last_order() == order
        r_host, s_host = t_r.clone().cpu(), (first + t_s).cpu()
    side.synchronize()
    same(r_host.numpy(), f"torch tensors, {order}")
    seeds[order] = r_host.numpy().view(np.uint32)[:, 3].copy()
    if not ((s_host.numpy() >= samples) & (s_host.numpy() <= samples * depth)).all():
        raise SystemExit(f"torch tensors, {order}: segment counts outside samples .. samples * depth")
    # allocated results come back as DeviceArrays, still on torch's stream
    with torch.cuda.stream(side):
        r, s = ctx.trace_film(t_q, samples, img_w, img_h, order=order)
        assert isinstance(r, rtx.DeviceArray) and s is None
        same(r.numpy().view(np.float32), f"DeviceArray out, {order}")
        r.free()
if not (seeds["given"] == seeds["cost"]).all():
    raise SystemExit("the seeds depend on the order")
ctx.set_stream(None)  # the context's own stream again
r, s = ctx.trace_film(queries, samples, img_w, img_h, order="cost", segments=True)
same(r.view(np.float32), "own stream again")
assert r.dtype == rtx.PATH_RESULT_DTYPE and (r["seed"].view(np.uint32) == seeds["given"]).all()
assert s.dtype == np.uint32 and (s == s_host.numpy()).all()
ctx.close()
print("ok")
