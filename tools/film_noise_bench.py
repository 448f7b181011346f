"""The price of the noise film at a bench config (default C3, 1024x768 @ 512 spp, HEAD NEE), in one
session: the spp samples as --passes passes of spp / passes (default 8 x 64) through

  * a plain film (tools/film_bench.py's "passes" row: the figure to compare with another build's),
  * a noise film (the accumulate pass also squares its sums into the moment plane),
  * a noise film with spt_film_noise_summary after every pass from the second on (what render_until
    does: two more kernels, a 40-byte copy and a host synchronisation per pass),

against the one-shot spt_render_async. Device time between two events on the stream and the host's
wall time around them (the summary synchronises, so the wall time is its real price), median of
--reps. Also the error map and one summary alone.

The accumulate kernel alone cannot be bracketed by events (it is enqueued inside the pass): run this
script under `rocprofv3 --kernel-trace --stats -- python tools/film_noise_bench.py` for the times of
film_accumulate_kernel<false> (plain) and <true> (with the moment plane), and of the summary's
film_noise_partials_kernel<UniformCount> and film_noise_total_kernel (an adaptive film launches the
<PixelCount> instantiations of the partials and the error-map kernel instead).

usage: python tools/film_noise_bench.py [--width W --height H --spp S --passes K --reps N --out F.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    spt = importlib.import_module("small-pathtracer_amd")
    w, h, spp = args.width, args.height, args.spp
    if spp % args.passes or args.passes < 2:
        raise SystemExit("--passes must divide --spp into at least two batches")
    batch = spp // args.passes
    p = spt.default_params(width=w, height=h, spp=spp, seed=1, device=0)
    cam = spt.Camera(aspect=w / h)
    prims = spt.cornell_scene()
    r, plain, noise = spt.Renderer(0), spt.Film(p, 0), spt.Film(p, 0)
    noise.enable_noise(batch)
    buf = torch.empty(w * h * 3, dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        ms, wall = [], []
        for _ in range(args.reps + 1):  # the first one warms up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": round(statistics.median(ms[1:]), 4), "min_ms": round(min(ms[1:]), 4),
                "max_ms": round(max(ms[1:]), 4), "wall_median_ms": round(statistics.median(wall[1:]), 4)}

    def passes(film, summary):
        def run():
            film.clear(stream)
            for k in range(args.passes):
                last = k == args.passes - 1
                film.render(r, prims, cam, p, k * batch, batch, buf.data_ptr() if last else 0, stream)
                if summary and k >= 1:
                    film.noise_summary(stream)
        return run

    res = {"config": {"width": w, "height": h, "spp": spp, "passes": args.passes, "batch": batch,
                      "reps": args.reps},
           "kernel_sources_sha16": spt.build_sources_sha16()}
    res["one_shot"] = timed(lambda: r.render_async(prims, cam, p, buf.data_ptr(), stream))
    r.stats()
    res["plain_film"] = timed(passes(plain, False))
    res["noise_film"] = timed(passes(noise, False))
    res["noise_film_summary_every_pass"] = timed(passes(noise, True))
    res["summary"] = timed(lambda: noise.noise_summary(stream))
    res["map"] = timed(lambda: noise.noise_map(buf.data_ptr(), stream))
    res["rmse"] = noise.noise_summary(stream)
    res["bytes"] = {"sums": w * h * 3 * 8, "m2": w * h * 3 * 16}
    for f in (plain, noise):
        f.close()
    r.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
