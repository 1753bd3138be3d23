"""One sigma per frame (blur_gaussian_*_frame_sigmas_batch_dev) against the loop over the scalar entry it replaces, and the scalar
entries themselves before and after the change.  Two builds of the library are compared in ONE session, alternating A/B/A/B, each
turn in a fresh process that loads its build through BLUR_AMD_LIB: `--base` (the build of the parent commit: tools/variant.sh keeps
builds under variants/) and the tree's own.  Times are HIP-event durations around windows of at least --window seconds of work,
after a warm-up of every shape; every turn takes --repeats windows per workload.

  loop64      64 u8 BGR frames of 224 x 224, sigmas uniform in [0.8, 2.5]: 64 scalar calls           (both builds)
  loop4k      8 u8 gray 4K frames, 8 different sigmas of window class 11: 8 scalar calls             (both builds)
  call64, call4k   the same work as ONE per-frame call                                                (the tree's build)
  scalar_u8, scalar_f32   8 x 4K gray u8 / 1-channel float32, sigma 20, one batch call of the scalar entry   (both builds)

One JSON line per turn, then a summary line: the one call against the base build's loop (fastest window), and the scalar entries'
median on the tree's build against the base build's slowest window.  DESIGN.md 2.7 holds the table.

  python tools/frame_sigmas_bench.py --base variants/parent/libblur_amd.so [--turns 2] [--repeats 3] [--window 0.25]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_windows(fn, window, repeats):
    """ms per call of fn: `repeats` windows of at least `window` seconds each, after a warm-up"""
    import torch
    fn()
    torch.cuda.synchronize()

    def run(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    reps = max(3, int(window * 1000.0 / max(run(3), 1e-3)) + 1)
    return [run(reps) for _ in range(repeats)]


def class_sigmas(B, rows, cols, nkb, count):
    """`count` different sigmas whose pads lie in window class nkb on this frame"""
    lo, hi = 8 * (nkb - 4) + 1, 8 * (nkb - 2)
    out, s = [], 0.5
    while len(out) < count and s < 100:
        pad = B.pffft_sizing(rows, cols, s)["pad"]
        if lo <= pad <= hi and (not out or pad != B.pffft_sizing(rows, cols, out[-1])["pad"]):
            out.append(s)
        s += 0.05
    assert len(out) == count
    return out


def turn(args):
    """one process, one build: every workload this build has"""
    import ctypes
    import torch                                      # first: the library then shares the HIP runtime torch has loaded (_lib.load)
    from blur_algorithms_amd import _lib
    probe = ctypes.CDLL(_lib.LIB_PATH)
    has_new = hasattr(probe, "blur_gaussian_u8_frame_sigmas_batch_dev")
    if not has_new:                                   # a build from before these entries: bind what it has
        for name in [n for n in _lib.SYMBOLS if "frame_sigmas" in n]:
            del _lib.SYMBOLS[name]
    import numpy as np
    import blur_algorithms_amd as B
    ctx = B.BlurContext(0)
    rng = np.random.default_rng(0)
    res = {"lib": os.path.relpath(_lib.LIB_PATH, ROOT), "per_frame_entries": has_new}

    def loop_and_call(name, frames, sigmas):
        x = torch.from_numpy(frames).cuda()
        y = torch.empty_like(x)

        def loop():
            for f, s in enumerate(sigmas):
                ctx.gaussian(x[f], s, out=y[f])
        res["loop" + name] = timed_windows(loop, args.window, args.repeats)
        if has_new:
            res["call" + name] = timed_windows(lambda: ctx.gaussian_per_frame(x, sigmas, out=y), args.window, args.repeats)
            res["family" + name] = ctx.last_engine()[0]

    loop_and_call("64", rng.integers(0, 256, (64, 224, 224, 3), dtype=np.uint8), [float(s) for s in rng.uniform(0.8, 2.5, 64)])
    loop_and_call("4k", rng.integers(0, 256, (8, 2160, 3840, 1), dtype=np.uint8), class_sigmas(B, 2160, 3840, 11, 8))
    x = torch.from_numpy(rng.integers(0, 256, (8, 2160, 3840, 1), dtype=np.uint8)).cuda()
    y = torch.empty_like(x)
    res["scalar_u8"] = timed_windows(lambda: ctx.gaussian(x, 20.0, out=y), args.window, args.repeats)
    xf = torch.from_numpy(rng.standard_normal((8, 2160, 3840, 1)).astype(np.float32)).cuda()
    yf = torch.empty_like(xf)
    res["scalar_f32"] = timed_windows(lambda: ctx.gaussian_f32(xf, 20.0, out=yf), args.window, args.repeats)
    ctx.close()
    print(json.dumps({k: ([round(t, 4) for t in v] if isinstance(v, list) else v) for k, v in res.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", help="libblur_amd.so of the parent commit")
    ap.add_argument("--turns", type=int, default=2, help="A/B pairs")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--turn", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.turn:
        return turn(args)
    if not args.base or not os.path.exists(args.base):
        sys.exit("--base: the parent commit's libblur_amd.so is needed (tools/variant.sh builds one under variants/)")
    tree = os.path.join(ROOT, "blur_algorithms_amd", "libblur_amd.so")
    got = {"base": [], "tree": []}
    for _ in range(args.turns):
        for which, lib in (("base", os.path.abspath(args.base)), ("tree", tree)):
            env = dict(os.environ, BLUR_AMD_LIB=lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--turn", "--repeats", str(args.repeats), "--window", str(args.window)],
                                 env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
            line = [l for l in out.splitlines() if l.startswith("{")][-1]
            print(which, line, flush=True)
            got[which].append(json.loads(line))
    pool = lambda which, key: [t for turn_ in got[which] for t in turn_.get(key, [])]
    summary = {}
    for name in ("64", "4k"):
        loop, call = pool("base", "loop" + name), pool("tree", "call" + name)
        summary["loop%s_base_fastest_ms" % name] = round(min(loop), 4)
        summary["call%s_median_ms" % name] = round(statistics.median(call), 4)
        summary["call%s_slowest_ms" % name] = round(max(call), 4)
        summary["loop_over_call_%s" % name] = round(min(loop) / statistics.median(call), 2)
        summary["call%s_faster_than_fastest_loop" % name] = max(call) < min(loop)
    for name in ("scalar_u8", "scalar_f32"):
        base, new = pool("base", name), pool("tree", name)
        summary[name + "_base_ms"] = [round(min(base), 4), round(statistics.median(base), 4), round(max(base), 4)]
        summary[name + "_tree_median_ms"] = round(statistics.median(new), 4)
        summary[name + "_within_1pct_of_base_slowest"] = statistics.median(new) <= 1.01 * max(base)
    print("summary", json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
