"""The price of progressive rendering at a bench config (default C3, 1024x768 @ 512 spp, HEAD NEE):

  * the spp samples as 1, 2, 4 and 8 film passes (each pass: render launch + accumulate), against the
    one-shot spt_render_async, device time between two events on the stream, median of --reps;
  * the film's resolve and merge alone, the same way.

The accumulate kernel alone cannot be bracketed by events (it is enqueued inside the pass): run this
script under `rocprofv3 --kernel-trace --stats -- python tools/film_bench.py` for the per-kernel times
of film_accumulate_kernel, film_resolve_kernel and film_merge_kernel.

usage: python tools/film_bench.py [--width W --height H --spp S --reps N --out FILE.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    spt = importlib.import_module("small-pathtracer_amd")
    w, h, spp = args.width, args.height, args.spp
    p = spt.default_params(width=w, height=h, spp=spp, seed=1, device=0)
    cam = spt.Camera(aspect=w / h)
    prims = spt.cornell_scene()
    r, film, other = spt.Renderer(0), spt.Film(p, 0), spt.Film(p, 0)
    buf = torch.empty(w * h * 3, dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        ms = []
        for _ in range(args.reps + 1):  # the first one warms up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": round(statistics.median(ms[1:]), 4), "min_ms": round(min(ms[1:]), 4),
                "max_ms": round(max(ms[1:]), 4)}

    res = {"config": {"width": w, "height": h, "spp": spp, "reps": args.reps},
           "kernel_sources_sha16": spt.build_sources_sha16()}
    res["one_shot"] = timed(lambda: r.render_async(prims, cam, p, buf.data_ptr(), stream))
    r.stats()
    res["passes"] = {}
    for k in (1, 2, 4, 8):
        windows = spt.sample_windows(spp, k)

        def run():
            film.clear(stream)
            for i, (base, count) in enumerate(windows):
                last = i == len(windows) - 1
                film.render(r, prims, cam, p, base, count, buf.data_ptr() if last else 0, stream)

        res["passes"][str(k)] = timed(run)
        kms = []
        film.clear(stream)
        for base, count in windows:  # the render kernels' own times, one pass at a time
            film.render(r, prims, cam, p, base, count, 0, stream)
            kms.append(round(r.stats()["kernel_ms"], 4))
        res["passes"][str(k)]["render_kernel_ms"] = kms
    res["resolve"] = timed(lambda: film.resolve(buf.data_ptr(), stream))
    other.clear(stream)
    res["merge"] = timed(lambda: (other.clear(stream), other.merge(film, stream)))
    res["clear"] = timed(lambda: other.clear(stream))
    nbytes = w * h * 3 * 8
    res["bytes"] = {"sums": nbytes, "floats": w * h * 3 * 4}
    for f in (film, other):
        f.close()
    r.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
