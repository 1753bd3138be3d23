"""1- and 4-channel Gaussian blur (blur_gaussian_u8_batch_dev) against what a caller has to do without it, timed with HIP events:
  c1: u8 -> f32 widening, blur_gaussian_f32c1_dev per frame, + 0.5f truncation back to u8 (torch ops for the conversions)
  c4: BGR + (A, A, A) split, two u8c3 batch calls, the frame put back together
and the u8c3 batch call on the same shape (time per frame as a fraction of it).  One JSON line per case.

  python tools/channels_bench.py [--reps 10]
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
    args = ap.parse_args()
    ctx = B.BlurContext(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    for (rows, cols, sigma) in ((2160, 3840, 20.0), (2160, 3840, 50.0), (1080, 1920, 20.0)):
        n = 8
        c3 = torch.randint(0, 256, (n, rows, cols, 3), dtype=torch.uint8, device="cuda", generator=g)
        o3 = torch.empty_like(c3)
        t3 = timed(lambda: ctx.pffft_(c3, sigma, out=o3), args.reps)
        for ch in (1, 4):
            x = torch.randint(0, 256, (n, rows, cols, ch), dtype=torch.uint8, device="cuda", generator=g)
            y = torch.empty_like(x)
            t_new = timed(lambda: ctx.gaussian(x, sigma, out=y), args.reps)
            fam = ctx.last_engine()[0]
            if ch == 1:
                def today():
                    f = x.view(n, rows, cols).float()
                    r = torch.empty_like(f)
                    for i in range(n):
                        ctx.pffft_plane(f[i], sigma, out=r[i])
                    y.view(n, rows, cols).copy_(((r + 0.5).to(torch.int32) & 255).to(torch.uint8))
            else:
                def today():
                    bgr = x[..., :3].contiguous()
                    aaa = x[..., 3:].expand(n, rows, cols, 3).contiguous()
                    ctx.pffft_(bgr, sigma)
                    ctx.pffft_(aaa, sigma)
                    y[..., :3] = bgr
                    y[..., 3:] = aaa[..., :1]
            t_old = timed(today, args.reps)
            gp = n * rows * cols / 1e6
            print(json.dumps(dict(rows=rows, cols=cols, sigma=sigma, frames=n, channels=ch, family=fam,
                                  ms_per_frame=round(t_new / n, 4), gps=round(gp / t_new, 2),
                                  today_ms_per_frame=round(t_old / n, 4), today_gps=round(gp / t_old, 2),
                                  u8c3_ms_per_frame=round(t3 / n, 4), fraction_of_u8c3=round(t_new / t3, 3),
                                  speedup_vs_today=round(t_old / t_new, 2))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
