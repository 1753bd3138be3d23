"""Gaussian blur of pitched frames and regions of interest (blur_gaussian_*_pitched_batch_dev) against what a caller had to do
without it, timed with HIP events, ms per call:
  today: view.contiguous(), the packed call on the copy, parent_view.copy_(result)       (three launches more, a second buffer)
  new:   the call on the view, in place
for u8 C = 4, u16 C = 1 and float32 C = 3; a 1080p region inside a 4K parent and a whole 1920-wide frame in a 2048-pixel pitch;
one frame and batches of 8.  One JSON line per case.

  python tools/pitched_bench.py [--reps 20]

--packed: the packed entries alone (u8 C = 1, 4 and float32 C = 1, 3, 4 at 4K and 1080p, sigma 20, 8 frames per call, ms per
frame), to compare two builds of the library on one machine (BLUR_AMD_LIB, or another checkout on PYTHONPATH).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not os.environ.get("BLUR_BENCH_NO_ROOT"):          # (set: take the package from PYTHONPATH, e.g. another checkout's)
    sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    fn()
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def make(kind, shape, g):
    import torch
    if kind == "u8":
        return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
    if kind == "u16":
        return torch.randint(0, 65536, shape, dtype=torch.int32, device="cuda", generator=g).to(torch.uint16)
    return torch.rand(shape, dtype=torch.float32, device="cuda", generator=g)


def packed(ctx, reps):
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    n, sigma = 8, 20.0
    for rows, cols in ((2160, 3840), (1080, 1920)):
        for kind, ch in (("u8", 1), ("u8", 4), ("f32", 1), ("f32", 3), ("f32", 4)):
            x = make(kind, (n, rows, cols, ch), g)
            y = torch.empty_like(x)
            fn = ctx.gaussian if kind == "u8" else ctx.gaussian_f32
            ts = [timed(lambda: fn(x, sigma, out=y), reps) / n for _ in range(3)]
            print(json.dumps({"case": "packed", "shape": [rows, cols], "type": kind, "channels": ch, "sigma": sigma, "frames": n,
                              "family": ctx.last_engine()[0], "ms_per_frame": [round(t, 5) for t in ts]}), flush=True)
            del x, y


def pitched(ctx, reps):
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    sigma = 20.0
    fns = {"u8": ctx.gaussian, "u16": ctx.gaussian_u16, "f32": ctx.gaussian_f32}
    for n in (1, 8):
        for kind, ch in (("u8", 4), ("u16", 1), ("f32", 3)):
            for name, pshape, y0, x0, rows, cols in (("1080p region of a 4K parent", (2160, 3840), 540, 960, 1080, 1920),
                                                      ("1920-wide frame in a 2048-pixel pitch", (1080, 2048), 0, 0, 1080, 1920)):
                parent = make(kind, (n,) + pshape + (ch,), g)
                view = parent[:, y0:y0 + rows, x0:x0 + cols]
                fn = fns[kind]

                def today():
                    c = view.view(torch.int16).contiguous().view(torch.uint16) if kind == "u16" else view.contiguous()
                    fn(c, sigma)
                    (view.view(torch.int16) if kind == "u16" else view).copy_(c.view(torch.int16) if kind == "u16" else c)
                t_old = timed(today, reps)
                t_new = timed(lambda: fn(view, sigma), reps)
                fam = ctx.last_engine()[0]
                print(json.dumps({"case": name, "type": kind, "channels": ch, "sigma": sigma, "frames": n, "family": fam,
                                  "today_ms": round(t_old, 4), "pitched_ms": round(t_new, 4), "ratio": round(t_old / t_new, 3)}), flush=True)
                del parent, view


def main():
    import blur_algorithms_amd as B
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--packed", action="store_true")
    args = ap.parse_args()
    ctx = B.BlurContext(0)
    (packed if args.packed else pitched)(ctx, args.reps)
    ctx.close()


if __name__ == "__main__":
    main()
