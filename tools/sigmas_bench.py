"""One sigma per channel (blur_gaussian_*_sigmas_batch_dev) against what a caller does without it, timed with HIP events, 8 frames
per call, the quirk on:
  new        the one call with the sequence of sigmas
  composed   one scalar call per distinct sigma > 0 into a temporary (without the gather), and the same plus the gather of one
             channel from each result into the destination (sigma 0: the source's channel)
  floor      the single scalar call with the largest sigma
One JSON line per case: ms per call, and new as a fraction of each.  DESIGN.md 2.5 holds the table.

  python tools/sigmas_bench.py [--reps 10] [--runs 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("u8", 3, (0.0, 11.0, 11.0)), ("u8", 3, (5.0, 5.0, 7.0)), ("u8", 4, (20.0, 20.0, 20.0, 0.0)), ("f32", 3, (3.0, 11.0, 11.0)),
         ("u16", 3, (3.0, 11.0, 11.0)))
SHAPES = ((2160, 3840), (1080, 1920))


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
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--frames", type=int, default=8)
    args = ap.parse_args()
    ctx = B.BlurContext(0)
    rng = np.random.default_rng(0)
    n = args.frames
    for rows, cols in SHAPES:
        for t, ch, sig in CASES:
            if t == "f32":
                x = torch.from_numpy(rng.standard_normal((n, rows, cols, ch)).astype(np.float32)).cuda()
            else:
                x = torch.from_numpy(rng.integers(0, 256 if t == "u8" else 65536, (n, rows, cols, ch), dtype=np.uint8 if t == "u8" else np.uint16)).cuda()
            fn = getattr(ctx, "gaussian" if t == "u8" else "gaussian_" + t)
            y = torch.empty_like(x)
            distinct = sorted(set(s for s in sig if s > 0))
            tmp = {s: torch.empty_like(x) for s in distinct}
            # (torch has few operators for uint16: the gather moves the samples as int16)
            raw = (lambda v: v.view(torch.int16)) if t == "u16" else (lambda v: v)

            def composed():
                for s in distinct:
                    fn(x, s, out=tmp[s])

            def gathered():
                composed()
                for c, s in enumerate(sig):
                    raw(y)[..., c] = raw(tmp[s] if s > 0 else x)[..., c]

            runs = []
            for _ in range(args.runs):
                runs.append((timed(lambda: fn(x, sig, out=y), args.reps), timed(composed, args.reps), timed(gathered, args.reps),
                             timed(lambda: fn(x, max(sig), out=y), args.reps)))
            fn(x, sig, out=y)
            fam = ctx.last_engine()[0]
            new, comp, gath, floor = (sorted(r[i] for r in runs) for i in range(4))
            print(json.dumps({"type": t, "channels": ch, "sigmas": sig, "rows": rows, "cols": cols, "frames": n, "family": fam,
                              "new_ms": [round(v, 3) for v in new], "composed_ms": [round(v, 3) for v in comp],
                              "composed_gather_ms": [round(v, 3) for v in gath], "floor_ms": [round(v, 3) for v in floor],
                              "composed_over_new": round(min(comp) / min(new), 3), "gathered_over_new": round(min(gath) / min(new), 3),
                              "new_over_floor": round(min(new) / min(floor), 3)}), flush=True)
            del x, y, tmp
    ctx.close()


if __name__ == "__main__":
    main()
