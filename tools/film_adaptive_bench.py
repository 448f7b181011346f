"""What adaptive sampling saves at a bench config (default C3, 1024x768 @ 512 spp, HEAD NEE), in one
session: render_until (every batch renders every pixel, the error map only decides when to stop)
against render_adaptive (after every pass the pixels whose standard error is at most the target
retire, the next pass renders the rest), for two targets; and against render_adaptive with the
pooled rule (a pixel retires on the error pooled over its (2R + 1)^2 neighbourhood,
spt_film_adaptive_select_pooled): R = 1, 2, 4 with and without the centre at --min-batches and
--threshold-scale, and R = 2 without the centre at min_batches 2 (--no-pool leaves these rows out).

The targets come from the run itself and are printed: R = the estimated RMSE (largest channel) of the
full uniform film, targets = --factors x R (default 1.5 and 1.15: a uniform render reaches them
after about 1 / 2.25 and 1 / 1.32 of its batches).

Per target and method: the pixel-samples spent, the time (the loop of render_until / render_adaptive
re-stated here on one Renderer and one film each, so that no allocation is timed: device time between two
events around the loop, which includes the host's summaries and selections, and the host's wall time;
median of --reps), the estimated RMSE at the stop and the TRUE RMSE of the resolved image against the
mean of --truth (16) independently seeded full-spp renders of this build. The truth's own noise adds
about 1 / (2 x 16) to a full render's RMSE (sqrt(1 + 1/16)); it is left in, the same for both methods.
"true2_x_samples" = true_rmse_all^2 x samples_of_full is the figure of merit: constant for a uniform
render, so a method beats the uniform film where it is lower at the same target.

usage: python tools/film_adaptive_bench.py [--width W --height H --spp S --batch B --min-batches M
                                            --threshold-scale X --factors 1.5,1.15 --truth 16
                                            --reps N --no-pool --out F.json]
--min-batches and --threshold-scale are render_adaptive's guards against retiring a pixel on a lucky
estimate: full batches before the first selection, and a retire threshold below the target.
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
    ap.add_argument("--batch", type=int, default=0, help="default spp / 16")
    ap.add_argument("--min-batches", type=int, default=4)
    ap.add_argument("--threshold-scale", type=float, default=1.0)
    ap.add_argument("--factors", default="1.5,1.15")
    ap.add_argument("--truth", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-pool", action="store_true", help="without the pooled-rule rows")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    spt = importlib.import_module("small-pathtracer_amd")
    w, h, spp = args.width, args.height, args.spp
    batch = args.batch or spp // 16
    nb = spp // batch
    need = max(2, args.min_batches)
    p = spt.default_params(width=w, height=h, spp=spp, seed=1, device=0)
    cam, prims = spt.Camera(aspect=w / h), spt.cornell_scene()
    buf = torch.empty(w * h * 3, dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    truth = np.zeros((h, w, 3), np.float64)
    for k in range(args.truth):
        q = spt.default_params(width=w, height=h, spp=spp, seed=1000 + k, device=0)
        truth += spt.render(prims, cam, q)
    truth /= args.truth

    # render_until runs on a noise film, render_adaptive on an adaptive one: what each costs
    r, uniform, film = spt.Renderer(0), spt.Film(p, 0), spt.Film(p, 0)
    uniform.enable_noise(batch)
    film.enable_noise(batch)
    film.enable_adaptive()

    def loop(target, adaptive, first=need, pool_radius=0, loo=False):
        """render_until / render_adaptive on its film -> the summary at the stop. first: the batches
        before the first summary; pool_radius, loo: the pooled rule (0: a pixel's own estimate)."""
        f = film if adaptive else uniform
        f.clear(stream)
        s = None
        for k in range(nb):
            f.render(r, prims, cam, p, k * batch, batch, 0, stream)
            r.stats()
            if k + 1 >= first:
                s = f.noise_summary(stream)
                if max(s["rmse"]) <= target:
                    break
                if adaptive and k + 1 < nb and \
                        f.adaptive_select(args.threshold_scale * target, None, stream, pool_radius, loo) == 0:
                    break
        f.resolve(buf.data_ptr(), stream)
        return s

    def measure(target, adaptive, first=need, pool_radius=0, loo=False):
        ms, wall = [], []
        for _ in range(args.reps + 1):  # the first one warms up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            s = loop(target, adaptive, first, pool_radius, loo)
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(e0.elapsed_time(e1))
        img = buf.cpu().numpy().reshape(h, w, 3).astype(np.float64)
        if adaptive:
            a = film.adaptive_info()
            cnt = film.counts_to_numpy() & np.uint32(spt.COUNT_MASK)
        else:
            front = uniform.noise_info()["batches_done"]
            a = {"samples_total": w * h * batch * front, "front": front, "n_active": w * h}
            cnt = np.full((h, w), front, np.uint32)
        err = np.sqrt(((img - truth) ** 2).mean(axis=(0, 1)))
        true_all = float(np.sqrt(((img - truth) ** 2).mean()))
        return {"samples": a["samples_total"], "samples_of_full": round(a["samples_total"] / (w * h * spp), 4),
                "front": a["front"], "n_active_at_stop": a["n_active"],
                "batches_min_mean_max": [int(cnt.min()), round(float(cnt.mean()), 3), int(cnt.max())],
                "device_ms": round(statistics.median(ms[1:]), 3),
                "wall_ms": round(statistics.median(wall[1:]), 3),
                "estimated_rmse": s["rmse"], "estimated_rmse_all": s["rmse_all"],
                "true_rmse": [float(x) for x in err],
                "true_rmse_all": true_all,
                "true_over_estimated_all": true_all / s["rmse_all"],
                "true2_x_samples": true_all ** 2 * a["samples_total"] / (w * h * spp)}

    full = loop(0.0, False)  # every batch: the full uniform film
    base = max(full["rmse"])
    targets = [float(f) * base for f in args.factors.split(",")]
    print("full film: estimated rmse", full["rmse"], "-> targets", targets, flush=True)
    res = {"config": {"width": w, "height": h, "spp": spp, "batch": batch, "batches": nb,
                      "min_batches": need, "threshold_scale": args.threshold_scale, "truth_renders": args.truth, "reps": args.reps},
           "kernel_sources_sha16": spt.build_sources_sha16(),
           "full_film": measure(0.0, False), "targets": []}
    pooled = [] if args.no_pool else \
        [(R, loo, need) for R in (1, 2, 4) for loo in (False, True)] + [(2, True, 2)]
    for f, t in zip(args.factors.split(","), targets):
        row = {"target": t, "factor_of_full_rmse": float(f),
               "render_until": measure(t, False),
               "render_adaptive": measure(t, True)}
        if pooled:
            row["render_adaptive_pooled"] = [
                dict({"pool_radius": R, "exclude_center": loo, "min_batches": first},
                     **measure(t, True, first, R, loo)) for R, loo, first in pooled]
        res["targets"].append(row)
        for name, m in [("render_until", row["render_until"]), ("adaptive", row["render_adaptive"])] + \
                [(f"pooled R={q['pool_radius']} loo={int(q['exclude_center'])} min={q['min_batches']}", q)
                 for q in row.get("render_adaptive_pooled", [])]:
            print(f"  {t:.4f} {name:26s} samples {m['samples_of_full']:.3f}  {m['device_ms']:7.2f} ms  est "
                  f"{m['estimated_rmse_all']:.4f}  true {m['true_rmse_all']:.4f}  ratio "
                  f"{m['true_over_estimated_all']:.3f}  true2 x samples {1e3 * m['true2_x_samples']:.3f}e-3",
                  flush=True)
    uniform.close()
    film.close()
    r.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
