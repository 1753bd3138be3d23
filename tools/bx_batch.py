"""tools/bx_batch.py -- fastboxblur k = 41, P = 3 on batches of RGB frames (GPU box): per-frame time of one batch call
(blur_fastboxblur_u8_batch_dev) against a loop of single calls, for 1080p / 4K / 8K and n = 1 / 8 / 64, then the chunk cap
(BLUR_BOX_CHUNK_MIB) swept on 64 x 4K.  Times are HIP events around the work on torch's stream, after a warm-up.

  python tools/bx_batch.py [--out results.json] [--sizes 1080p,4k,8k] [--ns 1,8,64] [--caps 32,64,128,256] [--only-vertical-trace]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import blur_algorithms_amd as B  # noqa: E402

SIZES = {"1080p": (1080, 1920), "4k": (2160, 3840), "8k": (4320, 7680)}
K, P = 41, 3


def timed(fn, reps):
    """ms per call of fn() (HIP events on the current stream; one warm-up call first)"""
    fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def reps_for(frame_bytes, n):
    # about 3 GB of frames per measurement window (a few hundred ms at the rates involved), at least 3 calls
    return max(3, int(3e9 / (frame_bytes * n)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="1080p,4k,8k")
    ap.add_argument("--ns", default="1,8,64")
    ap.add_argument("--caps", default="32,64,128,256")
    ap.add_argument("--only-vertical-trace", action="store_true", help="one batch call of 64 x 4K, for a kernel trace")
    a = ap.parse_args()
    ctx = B.BlurContext(0)
    ctx.use_torch_stream()
    if a.only_vertical_trace:
        x = torch.randint(0, 256, (64, 2160, 3840, 3), dtype=torch.uint8, device="cuda")
        for _ in range(3):
            ctx.fastboxblur_batch(x, K, P)
        torch.cuda.synchronize()
        print("64 x 4K batch: 3 calls done", flush=True)
        return
    rows = []
    for name in a.sizes.split(","):
        h, w = SIZES[name]
        fb = h * w * 3
        for n in (int(s) for s in a.ns.split(",")):
            x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
            reps = reps_for(fb, n)
            t_batch = timed(lambda: ctx.fastboxblur_batch(x, K, P), reps)

            def loop():
                for i in range(n):
                    ctx.fastboxblur(x[i], K, P)
            t_loop = timed(loop, reps)
            plan = B.fastboxblur_batch_plan(n, w, h, 3, K, P)
            r = {"size": name, "n": n, "batch_ms_per_frame": t_batch / n, "loop_ms_per_frame": t_loop / n,
                 "speedup": t_loop / t_batch, "frames_per_chunk": plan[0], "chunks": plan[1],
                 "batch_GBps_12Bpx": 12 * h * w * n / (t_batch * 1e-3) / 1e9}
            rows.append(r)
            print("%-5s n=%-3d batch %.4f ms/frame  loop %.4f ms/frame  x%.2f  (%d per chunk, %d chunks, %.0f GB/s of 12 B/px)"
                  % (name, n, r["batch_ms_per_frame"], r["loop_ms_per_frame"], r["speedup"], plan[0], plan[1], r["batch_GBps_12Bpx"]), flush=True)
            del x
            torch.cuda.empty_cache()
    caps = []
    if a.caps:
        h, w = SIZES["4k"]
        n = 64
        x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
        for cap in (int(s) for s in a.caps.split(",")):
            os.environ["BLUR_BOX_CHUNK_MIB"] = str(cap)
            plan = B.fastboxblur_batch_plan(n, w, h, 3, K, P)
            t = timed(lambda: ctx.fastboxblur_batch(x, K, P), reps_for(h * w * 3, n))
            caps.append({"cap_mib": cap, "frames_per_chunk": plan[0], "chunks": plan[1], "ms_per_frame": t / n})
            print("64 x 4K, cap %4d MiB: %d frames per chunk, %d chunks: %.4f ms/frame" % (cap, plan[0], plan[1], t / n), flush=True)
        os.environ.pop("BLUR_BOX_CHUNK_MIB", None)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"ksize": K, "passes": P, "sizes": rows, "cap_sweep": caps}, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
