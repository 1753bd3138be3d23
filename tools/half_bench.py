"""Gaussian blur of float16 / bfloat16 images of 1, 3 or 4 channels (blur_gaussian_f16_batch_dev, blur_gaussian_bf16_batch_dev)
against what a caller has to do without them, timed with HIP events, 8 frames per call, quirk on, ms per frame:
  today: widen to float32 (t.float()), BlurContext.gaussian_f32, narrow (.to(dtype)), in the same process on the same tensors
and beside both the f32 entry alone.  4K and 1080p at sigma 20, 4K at sigma 50.  One JSON line per case; `ratio` = new / today
(the aim at sigma 20 is <= 0.96).

  python tools/half_bench.py [--reps 10] [--runs 2]
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
    import torch
    import blur_algorithms_amd as B
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2, help="repeat every measurement; the range is reported")
    args = ap.parse_args()
    ctx = B.BlurContext(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    n = 8
    for (rows, cols, sigma) in ((2160, 3840, 20.0), (1080, 1920, 20.0), (2160, 3840, 50.0)):
        for ch in (1, 3, 4):
            xf = torch.rand((n, rows, cols, ch), device="cuda", generator=gen)
            yf = torch.empty_like(xf)
            for dtype, new in ((torch.float16, ctx.gaussian_f16), (torch.bfloat16, ctx.gaussian_bf16)):
                x = xf.to(dtype)
                y = torch.empty_like(x)

                def today():
                    f = x.float()
                    ctx.gaussian_f32(f, sigma, out=f)
                    y.copy_(f.to(dtype))

                rec = dict(rows=rows, cols=cols, sigma=sigma, frames=n, channels=ch, dtype=str(dtype).split(".")[-1])
                for name, fn in (("new", lambda: new(x, sigma, out=y)), ("today", today), ("f32", lambda: ctx.gaussian_f32(xf, sigma, out=yf))):
                    ts = [timed(fn, args.reps) / n for _ in range(args.runs)]
                    rec[name + "_ms_per_frame"] = [round(min(ts), 4), round(max(ts), 4)]
                    rec[name + "_family"] = ctx.last_engine()[0]
                rec["ratio"] = round(rec["new_ms_per_frame"][0] / rec["today_ms_per_frame"][0], 3)
                print(json.dumps(rec), flush=True)
                del x, y
            del xf, yf
    ctx.close()


if __name__ == "__main__":
    main()
