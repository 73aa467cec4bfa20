#!/usr/bin/env python3
"""rtx_fold_frames (k_fold_frames) against a device-to-device copy of the same bytes.

The fold streams (m + 3) * pixels * 16 bytes: m sums read, the accumulator read
and written, the image written. The yardstick is hipMemcpyAsync device to
device (torch's contiguous copy_) moving the same total, half read and half
written, in the same process on the same stream, the two alternating. Event
time over `--launches` launches after a warm-up, the median of `--reps` blocks.

  python tools/fold_bench.py [--width 1920 --height 1080] [--m 1 4 8]
                             [--launches 20] [--reps 5]   -> one JSON line
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytrace-we-gpu_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--m", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch

    import rtx

    px = args.width * args.height
    stream = torch.cuda.current_stream()
    ctx = rtx.Context(0, stream=stream.cuda_stream)
    out = []
    for m in args.m:
        sums = torch.rand((m, px, 4), device="cuda")
        accum = torch.zeros((px, 4), device="cuda")
        image = torch.empty((px, 4), device="cuda")
        total = (m + 3) * px * 16
        src = torch.rand((total // 8,), device="cuda")  # total / 2 bytes read, total / 2 written
        dst = torch.empty_like(src)

        def fold():
            ctx.fold_frames(accum.data_ptr(), sums.data_ptr(), m, px, px, 2 * m, image.data_ptr())

        def copy():
            dst.copy_(src)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(args.launches):
                fn()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) / args.launches

        for fn in (fold, copy):  # warm-up
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        f_ms, c_ms = [], []
        for _ in range(args.reps):  # alternating
            accum.zero_()
            f_ms.append(timed(fold))
            c_ms.append(timed(copy))
        f, c = statistics.median(f_ms), statistics.median(c_ms)
        out.append({"m": m, "bytes": total, "fold_ms": round(f, 5), "copy_ms": round(c, 5),
                    "fold_gb_s": round(total / f / 1e6, 1), "copy_gb_s": round(total / c / 1e6, 1),
                    "fold_over_copy": round(f / c, 3),
                    "fold_ms_min_max": [round(min(f_ms), 5), round(max(f_ms), 5)],
                    "copy_ms_min_max": [round(min(c_ms), 5), round(max(c_ms), 5)]})
    ctx.close()
    print(json.dumps({"width": args.width, "height": args.height, "launches": args.launches, "reps": args.reps,
                      "cases": out}))


if __name__ == "__main__":
    main()
