"""One sigma per frame for bfloat16 and uint16 batches and for an NV12 clip (blur_gaussian_{bf16,u16}_frame_sigmas_batch_dev,
blur_gaussian_nv12_frame_sigmas_batch_dev) against the loop over the scalar entry of the same build that each replaces.  One
process, one build; the loop and the one call alternate, --turns times, each turn --repeats windows of at least --window seconds
(frame_sigmas_bench.timed_windows: HIP-event durations after a warm-up).

  bf16_64     64 bfloat16 BGR frames of 224 x 224, sigmas uniform in [0.8, 2.5]: 64 calls of gaussian_bf16 / one call
  u16_4k      8 uint16 gray 4K frames, 8 different sigmas of window class 11: 8 calls of gaussian_u16 / one call
  nv12_1080p  an 8-frame 1080p NV12 clip, luma sigma ramping 2 .. 16 (chroma half of it): 8 calls of gaussian_nv12 / one call

One JSON line per turn, then a summary line: per row the loop's and the call's fastest, median and slowest window in ms and the range
of loop / call (slowest call against fastest loop .. fastest call against slowest loop).  DESIGN.md 2.7 and 2.8 hold the table.

  python tools/frame_sigmas_types_bench.py [--turns 3] [--repeats 3] [--window 0.25]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from frame_sigmas_bench import class_sigmas, timed_windows

ROWS = ("bf16_64", "u16_4k", "nv12_1080p")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=3, help="loop / call pairs per row")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25)
    args = ap.parse_args()
    import torch
    import numpy as np
    import blur_algorithms_amd as B
    ctx = B.BlurContext(0)
    rng = np.random.default_rng(0)
    work = {}

    x = torch.from_numpy(rng.random((64, 224, 224, 3), dtype=np.float32)).to(torch.bfloat16).cuda()
    y = torch.empty_like(x)
    s64 = [float(s) for s in rng.uniform(0.8, 2.5, 64)]
    work["bf16_64"] = (lambda: [ctx.gaussian_bf16(x[f], s, out=y[f]) for f, s in enumerate(s64)],
                       lambda: ctx.gaussian_bf16_per_frame(x, s64, out=y))

    g = torch.from_numpy(rng.integers(0, 65536, (8, 2160, 3840, 1), dtype=np.uint16)).cuda()
    go = torch.empty_like(g)
    s4k = class_sigmas(B, 2160, 3840, 11, 8)
    work["u16_4k"] = (lambda: [ctx.gaussian_u16(g[f], s, out=go[f]) for f, s in enumerate(s4k)],
                      lambda: ctx.gaussian_u16_per_frame(g, s4k, out=go))

    ly = torch.from_numpy(rng.integers(0, 256, (8, 1080, 1920), dtype=np.uint8)).cuda()
    luv = torch.from_numpy(rng.integers(0, 256, (8, 540, 960, 2), dtype=np.uint8)).cuda()
    oy, ouv = torch.empty_like(ly), torch.empty_like(luv)
    ramp = [2.0 + 2.0 * f for f in range(8)]
    work["nv12_1080p"] = (lambda: [ctx.gaussian_nv12(ly[f], luv[f], s, out=(oy[f], ouv[f])) for f, s in enumerate(ramp)],
                          lambda: ctx.gaussian_nv12_per_frame(ly, luv, ramp, out=(oy, ouv)))

    got = {name: {"loop": [], "call": []} for name in ROWS}
    for _ in range(args.turns):
        line = {}
        for name in ROWS:
            for which, fn in zip(("loop", "call"), work[name]):
                t = timed_windows(fn, args.window, args.repeats)
                got[name][which] += t
                line["%s_%s" % (name, which)] = [round(v, 4) for v in t]
            line[name + "_family"] = ctx.last_engine()[0]
        print(json.dumps(line), flush=True)
    ctx.close()
    summary = {}
    for name in ROWS:
        loop, call = got[name]["loop"], got[name]["call"]
        for which, t in (("loop", loop), ("call", call)):
            summary["%s_%s_ms" % (name, which)] = [round(min(t), 4), round(statistics.median(t), 4), round(max(t), 4)]
        summary[name + "_loop_over_call"] = [round(min(loop) / max(call), 2), round(max(loop) / min(call), 2)]
    print("summary", json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
