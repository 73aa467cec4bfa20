"""Child process of test_gpu_cast.py::test_torch_tensors_on_the_current_stream.

torch must own the process's HIP runtime before librtx loads,
so this runs in its own interpreter: torch first, then rtx. The rays are a
torch tensor made by torch work on a side stream, the context launches on that
stream (torch's current one), the outputs are torch tensors read back by
torch; afterwards the context goes back to its own stream and casts again into
its own buffers. argv[1]: a directory with rays.npy ((n, 8) float32),
want.npy (n rtx_ray_hit records) and spheres.npy. Prints "ok" or raises."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytrace-we-gpu_amd"))
import rtx  # noqa: E402

d = sys.argv[1]
rays = np.load(os.path.join(d, "rays.npy"))
want = np.load(os.path.join(d, "want.npy"))
sph = np.load(os.path.join(d, "spheres.npy"))
n = len(rays)
assert want.dtype == rtx.RAY_HIT_DTYPE and rays.shape == (n, 8)


def same(got, what):
    got = np.ascontiguousarray(got).view(rtx.RAY_HIT_DTYPE).reshape(-1)
    for f in ("t", "normal"):
        a, b = got[f], want[f]
        if not ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all():
            raise SystemExit(f"{what}: {f} differs")
    for f in ("index", "front_face", "reserved"):
        if not (got[f] == want[f]).all():
            raise SystemExit(f"{what}: {f} differs")


torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
ctx = rtx.Context(0)
ctx.upload_world(rtx.World(sph, np.zeros(len(sph), np.float32), np.zeros((len(sph), 4), np.float32), 1, 1))
side = torch.cuda.Stream(device=dev)
host = torch.from_numpy(rays.copy())
for order in ("given", "coherent"):
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream != 0
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        # torch work on the stream, then the cast over its result, then torch work on the cast's result
        t_rays = (host.to(dev, non_blocking=True).view(torch.int32) + 0).view(torch.float32)
        t_hits = torch.full((n, 8), -7, dtype=torch.int32, device=dev)
        t_occ = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
        got = ctx.cast(t_rays, order=order, hits=t_hits, occluded=t_occ)
        assert got[0] is t_hits and got[1] is t_occ and ctx.cast_last_order() == order
        hits_host, occ_host = t_hits.clone().cpu(), t_occ.clone().cpu()
    side.synchronize()
    same(hits_host.numpy(), f"torch tensors, {order}")
    if not (occ_host.numpy() == (want["index"] >= 0)).all():
        raise SystemExit(f"torch tensors, {order}: the occluded bytes differ")
    # allocated outputs come back as DeviceArrays, still on torch's stream
    with torch.cuda.stream(side):
        h, o = ctx.cast(t_rays, order=order)
        assert isinstance(h, rtx.DeviceArray) and o is None
        same(h.numpy(), f"DeviceArray out, {order}")
        h.free()
ctx.set_stream(None)  # the context's own stream again
h, o = ctx.cast(rays, order="coherent", occluded=True)
same(h, "own stream again")
assert (o == (want["index"] >= 0)).all()
ctx.close()
print("ok")
