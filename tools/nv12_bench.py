"""NV12 / P016 surfaces (blur_gaussian_nv12_batch_dev, blur_gaussian_p016_batch_dev) against the route they replace, and the scalar
one-channel entries before and after the change.  Two builds of the library are compared in ONE session, alternating A/B/A/B, each
turn in a fresh process that loads its build through BLUR_AMD_LIB: `--base` (the build of the parent commit: tools/variant.sh keeps
builds under variants/) and the tree's own.  Times are HIP-event durations around windows of at least --window seconds of work,
after a warm-up of every shape; every turn takes --repeats windows per workload (tools/frame_sigmas_bench.py: timed_windows).

Per format (nv12: uint8, p016: uint16) and size (1080p, 4K), one frame, sigma = (20, 10, 10), quirk on, in place:
  split_<fmt>_<size>   the route without these entries: the one-channel call on Y, Cb/Cr split into two planes (two strided device
                       copies), two one-channel calls, the planes interleaved again (two strided copies)          (both builds)
  planes_<fmt>_<size>  of that route, the three one-channel calls alone (what a caller with planar chroma pays)     (both builds)
  call_<fmt>_<size>    the same work as ONE call on the surface                                                  (the tree's build)
  bgr_<size>           the u8 BGR call (pffft_) on a frame of the same size, sigma 20, for scale                    (both builds)
  scalar_u8, scalar_u16   8 x 4K one-channel frames, sigma 20, one batch call of the scalar entry                   (both builds)

One JSON line per turn, then a summary line: the one call against the split route (medians, and the call's slowest window against
the route's fastest), and the scalar entries' median on the tree's build against the base build's own min .. max spread.
DESIGN.md 2.8 holds the table.

  python tools/nv12_bench.py --base variants/parent/libblur_amd.so [--turns 2] [--repeats 3] [--window 0.25]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from frame_sigmas_bench import timed_windows  # noqa: E402

SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840)}
SIGMAS = (20.0, 10.0, 10.0)


def turn(args):
    """one process, one build: every workload this build has"""
    import ctypes
    import torch                                      # first: the library then shares the HIP runtime torch has loaded (_lib.load)
    from blur_algorithms_amd import _lib
    probe = ctypes.CDLL(_lib.LIB_PATH)
    has_new = hasattr(probe, "blur_gaussian_nv12_batch_dev")
    if not has_new:                                   # a build from before these entries: bind what it has
        for name in [n for n in _lib.SYMBOLS if "_nv12_" in n or "_p016_" in n]:
            del _lib.SYMBOLS[name]
    import numpy as np
    import blur_algorithms_amd as B
    ctx = B.BlurContext(0)
    rng = np.random.default_rng(0)
    res = {"lib": os.path.relpath(_lib.LIB_PATH, ROOT), "nv12_entries": has_new}
    tw = lambda fn: timed_windows(fn, args.window, args.repeats)

    for fmt, dt, one in (("nv12", np.uint8, ctx.gaussian), ("p016", np.uint16, ctx.gaussian_u16)):
        for size, (rows, cols) in SIZES.items():
            y = torch.from_numpy(rng.integers(0, np.iinfo(dt).max + 1, (rows, cols), dtype=dt)).cuda()
            uv = torch.from_numpy(rng.integers(0, np.iinfo(dt).max + 1, (rows // 2, cols // 2, 2), dtype=dt)).cuda()
            cb, cr = torch.empty_like(uv[..., 0].contiguous()), torch.empty_like(uv[..., 0].contiguous())
            # (the strided copies on int16 views of the same bits: a dtype every copy kernel knows)
            sv = (lambda t: t) if dt == np.uint8 else (lambda t: t.view(torch.int16))

            def planes():
                one(y, SIGMAS[0])
                one(cb, SIGMAS[1])
                one(cr, SIGMAS[2])

            def split():
                sv(cb).copy_(sv(uv)[..., 0])
                sv(cr).copy_(sv(uv)[..., 1])
                planes()
                sv(uv)[..., 0].copy_(sv(cb))
                sv(uv)[..., 1].copy_(sv(cr))

            key = "%s_%s" % (fmt, size)
            res["split_" + key] = tw(split)
            res["planes_" + key] = tw(planes)
            if has_new:
                res["call_" + key] = tw(lambda: ctx.gaussian_nv12(y, uv, SIGMAS))
                res["family_" + key] = ctx.last_engine()[0]
    for size, (rows, cols) in SIZES.items():
        bgr = torch.from_numpy(rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)).cuda()
        res["bgr_" + size] = tw(lambda: ctx.pffft_(bgr, SIGMAS[0]))
    x = torch.from_numpy(rng.integers(0, 256, (8, 2160, 3840, 1), dtype=np.uint8)).cuda()
    out = torch.empty_like(x)
    res["scalar_u8"] = tw(lambda: ctx.gaussian(x, 20.0, out=out))
    x16 = torch.from_numpy(rng.integers(0, 65536, (8, 2160, 3840, 1), dtype=np.uint16)).cuda()
    out16 = torch.empty_like(x16)
    res["scalar_u16"] = tw(lambda: ctx.gaussian_u16(x16, 20.0, out=out16))
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
    med = statistics.median
    summary = {}
    for fmt in ("nv12", "p016"):
        for size in SIZES:
            key = "%s_%s" % (fmt, size)
            split, planes, call = pool("base", "split_" + key) + pool("tree", "split_" + key), pool("tree", "planes_" + key), pool("tree", "call_" + key)
            summary[key] = {"split_ms": round(med(split), 4), "planes_ms": round(med(planes), 4), "call_ms": round(med(call), 4),
                            "split_over_call": round(med(split) / med(call), 3), "call_slowest_below_split_fastest": max(call) < min(split)}
    for size in SIZES:
        summary["bgr_" + size + "_ms"] = round(med(pool("tree", "bgr_" + size)), 4)
    for name in ("scalar_u8", "scalar_u16", "bgr_4k"):
        base, new = pool("base", name), pool("tree", name)
        summary[name + "_base_min_med_max_ms"] = [round(min(base), 4), round(med(base), 4), round(max(base), 4)]
        summary[name + "_tree_median_ms"] = round(med(new), 4)
        summary[name + "_inside_base_spread"] = min(base) <= med(new) <= max(base) or med(new) < min(base)
    print("summary", json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
