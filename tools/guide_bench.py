"""What a guide pass costs (spt_guide_render_async, guide_kernel), in device time between two HIP
events on the stream, a warm-up first and the median of --reps:

  * C3's shape (HEAD, 1024x768 @ 512 spp): the guide pass beside the kernel_ms of the C3 render in the
    same process, alternating;
  * the 32-sphere scene at 1024x768 @ 256 spp (max_depth 16, as config 5): the same;
  * the K sweep: 64x48 @ 4096 spp, the host's choice of lanes per pixel against K = 1 forced. Forcing
    K is no part of the ABI: it needs the library of `make -C small-pathtracer_amd/csrc guide_bench`
    (build/libspt_guide_bench.so, -DSPT_GUIDE_BENCH), which this tool loads in a child process of its
    own (SPT_LIB). Without that library the sweep is reported as not measured.

A short pass is timed as --inner passes between the two events (each a clear and a launch).

usage: python tools/guide_bench.py [--reps N --inner M --out FILE.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BENCH_LIB = os.path.join(ROOT, "build", "libspt_guide_bench.so")


def _timed(torch, fn, reps, inner=1):
    ms = []
    for _ in range(reps + 1):  # the first one warms up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return {"median_ms": round(statistics.median(ms[1:]), 4), "min_ms": round(min(ms[1:]), 4),
            "max_ms": round(max(ms[1:]), 4)}


def _pair(spt, torch, prims, w, h, spp, reps, **kw):
    """A render and a guide pass of the same arguments, alternating."""
    p = spt.default_params(width=w, height=h, spp=spp, seed=1, device=0, **kw)
    cam = spt.Camera(aspect=w / h)
    r, g = spt.Renderer(0), spt.Guide(p, 0)
    buf = torch.empty(w * h * 3, dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    render_ms, guide_ms, kernel = [], [], None
    for i in range(reps + 1):
        r.render_async(prims, cam, p, buf.data_ptr(), stream)
        st = r.stats()
        kernel = r.kernel()
        g.clear(stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.render(r, prims, cam, p, 0, spp, stream)
        e1.record()
        torch.cuda.synchronize()
        if i:  # the first round warms up
            render_ms.append(st["kernel_ms"])
            guide_ms.append(e0.elapsed_time(e1))
    k = g.info()["lanes_per_pixel"]
    g.close()
    r.close()
    rm, gm = statistics.median(render_ms), statistics.median(guide_ms)
    return {"width": w, "height": h, "spp": spp, "render_kernel": kernel,
            "render_kernel_ms": {"median": round(rm, 4), "min": round(min(render_ms), 4),
                                 "max": round(max(render_ms), 4)},
            "guide_pass_ms": {"median": round(gm, 4), "min": round(min(guide_ms), 4),
                              "max": round(max(guide_ms), 4)},
            "lanes_per_pixel": k, "guide_over_render": round(gm / rm, 4)}


def _sweep(reps, inner):
    """The child's work (SPT_LIB = the bench library): host K against K = 1 at 64x48 @ 4096 spp."""
    import torch
    spt = importlib.import_module("small-pathtracer_amd")
    lib = spt.load_library()
    fn = lib.spt_guide_bench_render_k
    VP, I32 = ctypes.c_void_p, ctypes.c_int32
    fn.argtypes = [VP, VP, ctypes.POINTER(spt.spt_prim), I32, ctypes.POINTER(spt.spt_camera),
                   ctypes.POINTER(spt.spt_params), I32, I32, I32, VP]
    fn.restype = I32
    w, h, spp = 64, 48, 4096
    p = spt.default_params(width=w, height=h, spp=spp, seed=1, device=0)
    cam = spt.Camera(aspect=w / h)
    prims = spt.cornell_scene()
    arr = spt._scene_array(prims)
    r, g = spt.Renderer(0), spt.Guide(p, 0)
    stream = torch.cuda.current_stream().cuda_stream

    def host():
        g.clear(stream)
        g.render(r, prims, cam, p, 0, spp, stream)

    def forced(k):
        def run():
            g.clear(stream)
            spt._check(fn(r._ctx, g._g, arr, len(prims), ctypes.byref(cam._c), ctypes.byref(p), 0, spp, k,
                          VP(stream or None)))
        return run

    host()
    ref = g.to_numpy()
    k_host = g.info()["lanes_per_pixel"]
    out = {"width": w, "height": h, "spp": spp, "host_lanes_per_pixel": k_host, "by_k": {}}
    for rnd in range(2):  # alternating, twice: the spread between the rounds is the noise
        for k in (k_host, 1, 8):
            forced(k)()
            assert (g.to_numpy() == ref).all(), f"K = {k} changed the records"
            out["by_k"].setdefault(str(k), []).append(_timed(torch, forced(k), reps, inner))
        out.setdefault("host_choice", []).append(_timed(torch, host, reps, inner))
    m = lambda k: statistics.median(x["median_ms"] for x in out["by_k"][str(k)])  # noqa: E731
    out["k1_over_host_k"] = round(m(1) / m(k_host), 3)
    g.close()
    r.close()
    print("SWEEP " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--sweep-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.sweep_child:
        return _sweep(args.reps, args.inner)
    res = {"config": {"reps": args.reps, "inner": args.inner}}
    # the K sweep first, in its own process with the bench library (this one has not opened the GPU yet)
    if os.path.exists(BENCH_LIB):
        c = subprocess.run([sys.executable, os.path.abspath(__file__), "--sweep-child", "--reps",
                            str(args.reps), "--inner", str(args.inner)],
                           env=dict(os.environ, SPT_LIB=BENCH_LIB), capture_output=True, text=True, timeout=600)
        line = [ln for ln in c.stdout.splitlines() if ln.startswith("SWEEP ")]
        if c.returncode != 0 or not line:
            raise SystemExit("the K sweep failed:\n" + c.stdout[-2000:] + c.stderr[-2000:])
        res["k_sweep"] = json.loads(line[0][6:])
    else:
        res["k_sweep"] = "not measured: build/libspt_guide_bench.so is missing (make guide_bench)"
    import torch
    spt = importlib.import_module("small-pathtracer_amd")
    res["kernel_sources_sha16"] = spt.build_sources_sha16()
    res["c3"] = _pair(spt, torch, spt.cornell_scene(), 1024, 768, 512, args.reps)
    res["spheres32"] = _pair(spt, torch, spt.spheres32_scene(), 1024, 768, 256, args.reps, max_depth=16)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
