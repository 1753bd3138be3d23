"""Gaussian blur of float32 images of 1, 3 or 4 channels (blur_gaussian_f32_batch_dev) against what a caller has to do without
it, timed with HIP events, 8 frames per call, ms per frame:
  today: split every frame into planes, blur_gaussian_f32c1_dev per plane and frame, interleave the planes back (torch ops)
and the u8c1 fused frame on the same shape for scale.  The measured error against the float64 oracle (max |error| / max|x|) of
the first frame is reported too.  One JSON line per case.

  python tools/f32_bench.py [--reps 10] [--no-error]
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
    ap.add_argument("--no-error", action="store_true")
    args = ap.parse_args()
    ctx = B.BlurContext(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    n = 8
    for (rows, cols, sigma) in ((2160, 3840, 20.0), (2160, 3840, 50.0), (1080, 1920, 20.0)):
        u1 = torch.randint(0, 256, (n, rows, cols, 1), dtype=torch.uint8, device="cuda", generator=g)
        t_u8 = timed(lambda: ctx.gaussian(u1, sigma, out=torch.empty_like(u1)), args.reps)
        for ch in (1, 3, 4):
            x = torch.rand((n, rows, cols, ch), dtype=torch.float32, device="cuda", generator=g)
            y = torch.empty_like(x)
            t_new = timed(lambda: ctx.gaussian_f32(x, sigma, out=y), args.reps)
            fam = ctx.last_engine()[0]
            planes = torch.empty((ch, rows, cols), dtype=torch.float32, device="cuda")
            res = torch.empty_like(planes)
            z = torch.empty_like(x)

            def today():
                for i in range(n):
                    planes.copy_(x[i].permute(2, 0, 1))
                    for c in range(ch):
                        ctx.pffft_plane(planes[c], sigma, out=res[c])
                    z[i].copy_(res.permute(1, 2, 0))
            t_old = timed(today, args.reps)
            rec = dict(rows=rows, cols=cols, sigma=sigma, frames=n, channels=ch, family=fam,
                       ms_per_frame=round(t_new / n, 4), today_ms_per_frame=round(t_old / n, 4),
                       speedup_vs_today=round(t_old / t_new, 2), u8c1_ms_per_frame=round(t_u8 / n, 4),
                       fraction_of_u8c1=round(t_new / t_u8, 2))
            if not args.no_error:
                from oracle import oracle as O
                img = x[0].cpu().numpy()
                got = y[0].cpu().numpy().astype(np.float64)
                err = max(float(np.max(np.abs(got[..., c] - O.pffft_plane_f64(img[..., c], sigma, True)))) for c in range(ch))
                rec["max_err_rel"] = float("%.3g" % (err / float(np.max(np.abs(img)))))
            print(json.dumps(rec), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
