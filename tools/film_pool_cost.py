"""The kernels of a pooled selection beside the ones with the same input traffic, for a run under
`rocprofv3 --kernel-trace --stats -- python tools/film_pool_cost.py`: on a C3-sized adaptive film
(1024x768, HEAD NEE, 4 batches of 32 of 512 spp) --reps times each: the error map
(film_noise_map_kernel), the unpooled selection (film_adapt_mark_kernel + the compaction), the pooled
map and the pooled selection at --radius (film_pool_rows_kernel, film_pool_map_kernel,
film_pool_mark_kernel). The threshold retires nothing that matters: every selection runs on a film set
back to the same counts, so each repetition does the same work.

usage: python tools/film_pool_cost.py [--width W --height H --radius R --reps N]
"""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    spt = importlib.import_module("small-pathtracer_amd")
    w, h, spp, batch = args.width, args.height, 512, 32
    p = spt.default_params(width=w, height=h, spp=spp, seed=1, device=0)
    cam, prims = spt.Camera(aspect=w / h), spt.cornell_scene()
    r, film = spt.Renderer(0), spt.Film(p, 0)
    film.enable_noise(batch)
    film.enable_adaptive()
    for k in range(4):
        film.render(r, prims, cam, p, k * batch, batch)
        r.stats()
    se = torch.empty(w * h * 3, dtype=torch.float32, device="cuda:0")
    counts = film.counts_to_numpy()
    thr = float(np.median(film.noise_map().max(axis=-1)))
    for _ in range(args.reps):
        film.noise_map(se.data_ptr())
        film.noise_pool_map(args.radius, False, se.data_ptr())
        for R, loo in ((0, False), (args.radius, False), (args.radius, True)):
            n = film.adaptive_select(thr, None, 0, R, loo)
            film.counts_from_numpy(counts)
    torch.cuda.synchronize()
    print(f"film_pool_cost: {w}x{h}, radius {args.radius}, threshold {thr:.5f}, last selection kept {n} "
          f"of {w * h}; {args.reps} repetitions")
    film.close()
    r.close()


if __name__ == "__main__":
    main()
