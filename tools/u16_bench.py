"""Gaussian blur of u16 images of 1, 3 or 4 channels (blur_gaussian_u16_batch_dev) against what a caller has to do without it,
timed with HIP events, 8 frames per call, quirk on, ms per frame:
  today: widen to float32 (torch), BlurContext.gaussian_f32, + 0.5, truncate, keep the low 16 bits, narrow to uint16 (torch)
and beside both the f32 entry alone and the u8 entry on the same shape.  One JSON line per case.

  python tools/u16_bench.py [--reps 10] [--runs 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    import numpy as np
    import torch
    import blur_algorithms_amd as B
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2, help="repeat every measurement; the range is reported")
    args = ap.parse_args()
    ctx = B.BlurContext(0)
    rng = np.random.default_rng(0)
    n = 8
    for (rows, cols, sigma) in ((2160, 3840, 20.0), (2160, 3840, 50.0), (1080, 1920, 20.0)):
        for ch in (1, 3, 4):
            x = torch.from_numpy(rng.integers(0, 65536, (n, rows, cols, ch), dtype=np.uint16)).cuda()
            y = torch.empty_like(x)
            xf = x.float()
            yf = torch.empty_like(xf)
            u8 = torch.from_numpy(rng.integers(0, 256, (n, rows, cols, ch), dtype=np.uint8)).cuda()
            y8 = torch.empty_like(u8)

            def today():
                f = x.float()
                ctx.gaussian_f32(f, sigma, out=f)
                y.copy_(((f + 0.5).to(torch.int32) & 0xffff).to(torch.uint16))

            rec = dict(rows=rows, cols=cols, sigma=sigma, frames=n, channels=ch)
            for name, fn in (("u16", lambda: ctx.gaussian_u16(x, sigma, out=y)), ("today", today),
                             ("f32", lambda: ctx.gaussian_f32(xf, sigma, out=yf)), ("u8", lambda: ctx.gaussian(u8, sigma, out=y8))):
                ts = [timed(fn, args.reps) / n for _ in range(args.runs)]
                rec[name + "_ms_per_frame"] = [round(min(ts), 4), round(max(ts), 4)]
                rec[name + "_family"] = ctx.last_engine()[0]
            rec["speedup_vs_today"] = round(rec["today_ms_per_frame"][0] / rec["u16_ms_per_frame"][0], 2)
            print(json.dumps(rec), flush=True)
            del x, y, xf, yf, u8, y8
    ctx.close()


if __name__ == "__main__":
    main()
