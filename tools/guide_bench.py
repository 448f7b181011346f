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

--chain (SPT_HAS_GUIDE_CHAIN): instead of the above, a chain guide pass (SPT_GUIDE_THROUGH_SPECULAR)
beside a first-hit pass, alternating in one process, at 1024x768 on the two specular scenes
(mirror_glass and cornell_specular @ 64 spp) and at C3's shape (HEAD has no specular primitive: the
chain pass does the same traces), 20 runs after 5 warm-ups, medians with min-max, and the ratio. With
--parent-tree DIR (a built checkout of the parent commit) the first-hit pass and the chain pass of this
tree and of the parent's library are timed in alternating child processes, --rounds of them each, to
show that neither moved: the parent is the yardstick, never this build against itself. A pass counts as
unchanged when the median of this tree's rounds exceeds the parent's by no more than the parent's own
min-max spread over its rounds.

--light (SPT_HAS_GUIDE_LIGHT): a light-guide pass (spt_light_guide_render_async) of either kind beside a
first-hit guide pass and a chain guide pass of the same build, all four alternating in one process, at
the --chain leg's shapes and with its protocol; the ratios are to the guide pass of the same kind.
mirror_glass has no light rectangle: its light guide samples a 24 x 24 square of the light sphere's
cap (prim 8). --parent-tree DIR times the two guide passes against the parent's library as --chain does.

usage: python tools/guide_bench.py [--reps N --inner M --out FILE.json]
       python tools/guide_bench.py --chain [--parent-tree DIR --rounds R] [--out FILE.json]
       python tools/guide_bench.py --light [--parent-tree DIR --rounds R] [--out FILE.json]
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


CHAIN_SHAPES = [("mirror_glass", 1024, 768, 64, dict(nee_prob=0.0)), ("cornell_specular", 1024, 768, 64, {}),
                ("c3_head", 1024, 768, 512, {})]
CHAIN_RUNS, CHAIN_WARM = 20, 5


def _scene_of(spt, name):
    return {"mirror_glass": spt.smallpt_mirror_glass_scene, "cornell_specular": spt.cornell_specular_scene,
            "c3_head": spt.cornell_scene}[name]()


def _stat(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def _pass_ms(torch, g, r, prims, cam, p, stream):
    g.clear(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.render(r, prims, cam, p, 0, p.spp, stream)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _chain_pairs(spt, torch):
    """A chain pass and a first-hit pass of the same arguments, alternating in this process."""
    out = {}
    for name, w, h, spp, kw in CHAIN_SHAPES:
        prims = _scene_of(spt, name)
        p = spt.default_params(width=w, height=h, spp=spp, seed=1, device=0, **kw)
        cam = spt.Camera(aspect=w / h)
        r = spt.Renderer(0)
        first, chain = spt.Guide(p, 0), spt.Guide(p, 0, through_specular=True)
        stream = torch.cuda.current_stream().cuda_stream
        ms = {"first_hit": [], "chain": []}
        for i in range(CHAIN_WARM + CHAIN_RUNS):
            for key, g in (("first_hit", first), ("chain", chain)):
                t = _pass_ms(torch, g, r, prims, cam, p, stream)
                if i >= CHAIN_WARM:
                    ms[key].append(t)
        hits = {k: int(g.to_numpy()[..., 7].sum()) for k, g in (("first_hit", first), ("chain", chain))}
        out[name] = {"width": w, "height": h, "spp": spp, "first_hit_ms": _stat(ms["first_hit"]),
                     "chain_ms": _stat(ms["chain"]), "lanes_per_pixel": first.info()["lanes_per_pixel"],
                     "chain_over_first_hit": round(statistics.median(ms["chain"]) /
                                                   statistics.median(ms["first_hit"]), 4),
                     "hits": hits}
        first.close()
        chain.close()
        r.close()
    return out


def _light_params(name, p):
    """The light a light guide of scene `name` samples: the parameters' rectangle, or for the classic
    box a square of the light sphere's cap (prim 8, centred (50, 81.6) at the ceiling)."""
    if name == "mirror_glass":
        p.light_id = 8
        p.light_x0, p.light_dx, p.light_z0, p.light_dz = 38.0, 24.0, 69.6, 24.0
        p.light_y, p.light_area = 81.6, 576.0
    return p


def _light_passes(spt, torch):
    """The two guide passes and the two light-guide passes of the same arguments, alternating."""
    out = {}
    for name, w, h, spp, kw in CHAIN_SHAPES:
        prims = _scene_of(spt, name)
        p = _light_params(name, spt.default_params(width=w, height=h, spp=spp, seed=1, device=0, **kw))
        cam = spt.Camera(aspect=w / h)
        r = spt.Renderer(0)
        objs = (("first_hit", spt.Guide(p, 0)), ("chain", spt.Guide(p, 0, through_specular=True)),
                ("light", spt.LightGuide(p, 0)), ("light_chain", spt.LightGuide(p, 0, through_specular=True)))
        stream = torch.cuda.current_stream().cuda_stream
        ms = {k: [] for k, _ in objs}
        for i in range(CHAIN_WARM + CHAIN_RUNS):
            for key, g in objs:
                t = _pass_ms(torch, g, r, prims, cam, p, stream)
                if i >= CHAIN_WARM:
                    ms[key].append(t)
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec = {k: g.to_numpy() for k, g in objs[2:]}
        out[name] = {"width": w, "height": h, "spp": spp, **{k + "_ms": _stat(v) for k, v in ms.items()},
                     "lanes_per_pixel": {k: g.info()["lanes_per_pixel"] for k, g in objs},
                     "light_over_first_hit": round(med["light"] / med["first_hit"], 4),
                     "light_chain_over_chain": round(med["light_chain"] / med["chain"], 4),
                     "chain_over_first_hit": round(med["chain"] / med["first_hit"], 4),
                     "samples": w * h * spp,
                     "tested": {k: int(v[..., 0].sum()) for k, v in rec.items()},
                     "lit": {k: int(v[..., 1].sum()) for k, v in rec.items()}}
        for _, g in objs:
            g.close()
        r.close()
    return out


def _passes_child(tree):
    """One child's work: the first-hit and the chain pass of the package under `tree` at every shape."""
    sys.path.insert(0, tree)
    import torch
    spt = importlib.import_module("small-pathtracer_amd")
    assert os.path.abspath(spt.LIB_PATH).startswith(os.path.abspath(tree)), spt.LIB_PATH
    out = {"kernel_sources_sha16": spt.build_sources_sha16()}
    for name, w, h, spp, kw in CHAIN_SHAPES:
        prims = _scene_of(spt, name)
        p = spt.default_params(width=w, height=h, spp=spp, seed=1, device=0, **kw)
        cam = spt.Camera(aspect=w / h)
        stream = torch.cuda.current_stream().cuda_stream
        out[name] = {}
        for key, chain in (("first_hit", False), ("chain", True)):
            r, g = spt.Renderer(0), spt.Guide(p, 0, through_specular=chain)
            out[name][key] = [_pass_ms(torch, g, r, prims, cam, p, stream)
                              for _ in range(CHAIN_WARM + CHAIN_RUNS)][CHAIN_WARM:]
            g.close()
            r.close()
    print("PASSES " + json.dumps(out))


def _against_parent(parent_tree, rounds):
    """This tree's first-hit and chain passes and the parent's, in alternating child processes."""
    runs = {"here": [], "parent": []}
    for _ in range(rounds):
        for key, tree in (("here", ROOT), ("parent", os.path.abspath(parent_tree))):
            env = {k: v for k, v in os.environ.items() if k != "SPT_LIB"}
            c = subprocess.run([sys.executable, os.path.abspath(__file__), "--passes-child", tree],
                               env=env, capture_output=True, text=True, timeout=300)
            line = [ln for ln in c.stdout.splitlines() if ln.startswith("PASSES ")]
            if c.returncode != 0 or not line:
                raise SystemExit(f"the {key} child failed:\n" + c.stdout[-2000:] + c.stderr[-2000:])
            runs[key].append(json.loads(line[0][7:]))
    out = {"rounds": rounds, "sha16": {k: v[0]["kernel_sources_sha16"] for k, v in runs.items()}}
    for name, *_ in CHAIN_SHAPES:
        out[name] = {}
        for kind in ("first_hit", "chain"):
            here = [statistics.median(x[name][kind]) for x in runs["here"]]
            par = [statistics.median(x[name][kind]) for x in runs["parent"]]
            over, spread = statistics.median(here) - statistics.median(par), max(par) - min(par)
            out[name][kind] = {"here_ms": _stat(here), "parent_ms": _stat(par),
                               "per_round_here": [round(v, 4) for v in here],
                               "per_round_parent": [round(v, 4) for v in par],
                               "here_over_parent": round(statistics.median(here) / statistics.median(par), 4),
                               "here_minus_parent_ms": round(over, 4), "parent_spread_ms": round(spread, 4),
                               "unchanged": over <= spread}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--sweep-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--chain", action="store_true", help="chain guide passes beside first-hit passes")
    ap.add_argument("--light", action="store_true", help="light-guide passes beside the guide passes")
    ap.add_argument("--parent-tree", default="", help="with --chain / --light: a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes-child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.sweep_child:
        return _sweep(args.reps, args.inner)
    if args.passes_child:
        return _passes_child(args.passes_child)
    if args.chain or args.light:
        res = {"config": {"runs": CHAIN_RUNS, "warm_ups": CHAIN_WARM}}
        # the children first: this process has not opened the GPU yet
        res["against_parent"] = (_against_parent(args.parent_tree, args.rounds) if args.parent_tree
                                 else "not measured: no --parent-tree")
        import torch
        spt = importlib.import_module("small-pathtracer_amd")
        res["kernel_sources_sha16"] = spt.build_sources_sha16()
        if args.light:
            res["light_beside_guides"] = _light_passes(spt, torch)
        else:
            res["chain_beside_first_hit"] = _chain_pairs(spt, torch)
        print(json.dumps(res))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
        return
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
