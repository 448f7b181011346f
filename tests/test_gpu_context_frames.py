"""What an spt_context carries from one frame to the next, observed: different frames back to back
on one context -- pipelined with no host synchronisation, synchronised, changed in one input at a
time, around rejected calls, mixed with the passes of plain, noise and adaptive films, on two streams
and two contexts -- and spt_render from four threads. The frames, the orders and the one-input chain
are tests/frame_cases.py (checked on the CPU by tests/test_context_frames.py).

The truth of every frame is the CPU oracle's image and statistics, computed once per module. Every
output buffer is rows * w * 3 + 1 floats filled with NaN before the frame is enqueued; the last float
is a guard and must still be NaN. Images are compared on their bits: there is nothing to tolerate.

The chain has no `light_id` link: no scene of this package has a second emitter that spt_params'
light lattice describes (frame_cases.chain).

Each test names the one-line change in spt_context.cpp or spt_film.hip that makes it fail
("Bites:"); HISTORY.md (round 17) says which of them were tried on the GPU, with a library built
from a scratch copy of the sources.
"""
import ctypes
import threading

import numpy as np
import pytest

import frame_cases as fc
from test_gpu_film import film_passes
from test_gpu_film_noise import m2_ints
from test_gpu_film_pool import planes_at, uniform_reference

pytestmark = pytest.mark.gpu

RETIRED, MASK = np.uint32(0x80000000), np.uint32(0x7FFFFFFF)
# the late rejection: 4096 x 4096 pixels x 128 one-sample units = 2^31 work units (plan_launch's text)
LATE, LATE_P = "too many work units; raise chunk", dict(width=4096, height=4096, spp=128, chunk=1)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def table(spt, oracle):
    """-> ({label: Frame}, {label: (oracle image, oracle statistics)}), computed once."""
    frames = fc.frames(spt)
    return frames, {k: f.truth(oracle) for k, f in frames.items()}


@pytest.fixture(scope="module")
def links(spt, oracle):
    """-> [(what changed, Frame, oracle image, oracle statistics)] of the one-input chain."""
    return [(what, f) + f.truth(oracle) for what, f in fc.chain(spt)]


def nan_buffer(torch, fr):
    return torch.full((fr.n_values + 1,), float("nan"), dtype=torch.float32, device="cuda:0")


def enqueue(r, fr, buf, stream):
    r.render_async(fr.prims, fr.cam, fr.p, buf.data_ptr(), stream)
    assert r.kernel() == fr.kernel, (fr.label, r.kernel(), fr.kernel)


def assert_image(buf, img, what):
    got = buf.cpu().numpy()
    assert np.isnan(got[-1]), f"{what}: the guard behind the image was written"
    a, b = got[:-1].view(np.uint32), img.reshape(-1).view(np.uint32)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, f"{what}: {bad.size} of {b.size} values differ, first at {bad[:5].tolist()}"


def assert_stats(spt, st, want, what):
    got = {k: st[k] for k in spt.STAT_KEYS}
    assert got == want, (what, got, want)


def play(spt, torch, r, seq, streams, synchronised, truth_of):
    """Enqueue seq = [(what, Frame)] on one context, frame i on streams[i % len(streams)], every
    frame into a buffer of its own; the caller's order between two streams is an event recorded
    after each enqueue that the next frame's stream waits for. synchronised: stats() after every
    frame, each the oracle's; else one stats() after the last enqueue, the last frame's. Then every
    buffer is its oracle image behind an intact guard."""
    bufs = [nan_buffer(torch, fr) for _, fr in seq]
    torch.cuda.synchronize()  # the fills, before another stream writes the buffers
    event = None
    for i, ((what, fr), buf) in enumerate(zip(seq, bufs)):
        s = streams[i % len(streams)]
        if len(streams) > 1 and event is not None:
            s.wait_event(event)
        enqueue(r, fr, buf, s.cuda_stream)
        if len(streams) > 1:
            event = torch.cuda.Event()
            event.record(s)
        if synchronised:
            st = r.stats()
            assert_stats(spt, st, truth_of(what)[1], f"frame {i} ({what})")
            if fr.rows:
                assert st["kernel_ms"] > 0, (i, what)
            else:
                assert st["samples"] == 0, (i, what)
    if not synchronised:
        assert_stats(spt, r.stats(), truth_of(seq[-1][0])[1], f"the last frame ({seq[-1][0]})")
    torch.cuda.synchronize()
    for i, ((what, fr), buf) in enumerate(zip(seq, bufs)):
        assert_image(buf, truth_of(what)[0], f"frame {i} ({what})")
    return bufs


def closing(torch, *things):
    """Wait for the device, then close contexts and films (none is destroyed with work in flight)."""
    torch.cuda.synchronize()
    for t in things:
        t.close()


@pytest.mark.parametrize("order", ["A", "B"])
def test_pipelined_sequence(spt, torch_dev, table, order):
    """One context, the current stream, no stats() and no synchronisation between the frames.
    Bites: drop the hipMemsetAsync of c->accum (`steal` is played twice, and its second launch adds
    to the first one's sums); skip the scene upload when n_prims is unchanged."""
    torch = torch_dev
    frames, truth = table
    seq = [(k, frames[k]) for k in fc.ORDERS[order](frames)]
    r = spt.Renderer(0)
    try:
        play(spt, torch, r, seq, [torch.cuda.current_stream()], False, truth.__getitem__)
    finally:
        closing(torch, r)


@pytest.mark.parametrize("order", ["A", "B"])
def test_synchronised_sequence(spt, torch_dev, table, order):
    """The same orders with stats() after every frame: each is that frame's, across `empty` and
    across a NEE -> cosine change.
    Bites: let c->nee_by_identity survive a launch (`|=` in place of its assignment: the cosine
    frame behind a HEAD NEE one in order A then reports nee_events = vertices - samples); drop
    `c->samples = 0` on the path of a shard without rows."""
    torch = torch_dev
    frames, truth = table
    seq = [(k, frames[k]) for k in fc.ORDERS[order](frames)]
    r = spt.Renderer(0)
    try:
        play(spt, torch, r, seq, [torch.cuda.current_stream()], True, truth.__getitem__)
    finally:
        closing(torch, r)


@pytest.mark.parametrize("synchronised", [False, True], ids=["pipelined", "synchronised"])
def test_one_input_changes(spt, torch_dev, links, synchronised):
    """head_nee at 32x24 @ 8, then frames that differ from the one before in exactly one input, then
    the first frame again, twice: what a "skip the upload when nothing changed" has to survive.
    Bites: skip the two scene hipMemcpyAsync when n_prims == c->n_prims (the light's emission, the
    wall's colour, the moved box and the edited light all keep 17 primitives); skip the d_kp
    upload when width, height and spp are unchanged."""
    torch = torch_dev
    by_name = {what: (img, st) for what, _, img, st in links}
    seq = [(what, fr) for what, fr, _, _ in links]
    r = spt.Renderer(0)
    try:
        bufs = play(spt, torch, r, seq, [torch.cuda.current_stream()], synchronised,
                    by_name.__getitem__)
        assert torch.equal(bufs[-1][:-1].view(torch.int32), bufs[-2][:-1].view(torch.int32))
        assert torch.equal(bufs[-1][:-1].view(torch.int32), bufs[0][:-1].view(torch.int32))
    finally:
        closing(torch, r)


def test_rejected_calls_in_mid_pipeline(spt, torch_dev, table):
    """Calls that validate rejects, between two frames in flight and again behind the second: each
    raises, queues nothing and leaves kernel() and stats() at the last good frame.
    Bites: set `c->last_kv = -1` (or c->samples) before validate() instead of after it."""
    torch = torch_dev
    frames, truth = table
    a, b, x = frames["upbox"], frames["spheres"], frames["specular"]
    stream = torch.cuda.current_stream().cuda_stream
    r = spt.Renderer(0)

    def with_p(**kw):
        q = spt.spt_params.from_buffer_copy(x.p)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    try:
        buf_a, buf_b, spare = nan_buffer(torch, a), nan_buffer(torch, b), nan_buffer(torch, x)
        calls = {
            "spp=0": lambda: r.render_async(x.prims, x.cam, with_p(spp=0), spare.data_ptr(), stream),
            "width=0": lambda: r.render_async(x.prims, x.cam, with_p(width=0), spare.data_ptr(), stream),
            "n_prims": lambda: r.render_async(list(x.prims) * 8, x.cam, x.p, spare.data_ptr(), stream),
            "light_id": lambda: r.render_async(x.prims, x.cam, with_p(light_id=len(x.prims)),
                                               spare.data_ptr(), stream),
            "null output": lambda: r.render_async(x.prims, x.cam, x.p, 0, stream),
            # a late rejection: validate accepts it, plan_launch counts 2^24 pixels x 128 one-sample
            # units = 2^31 and refuses on host arithmetic alone, before anything is allocated
            LATE: lambda: r.render_async(x.prims, x.cam, with_p(**LATE_P), spare.data_ptr(), stream),
        }
        assert len(x.prims) * 8 > 64 and x.p.nee_prob > 0
        enqueue(r, a, buf_a, stream)
        for last in (a, b):
            for what, call in calls.items():
                with pytest.raises(spt.SptError) as e:
                    call()
                assert e.value.status == 1, what
                if what == LATE:
                    assert str(e.value).split(": ", 1)[1] == LATE, str(e.value)
                assert r.kernel() == last.kernel, (what, r.kernel())
            if last is a:
                enqueue(r, b, buf_b, stream)
        assert_stats(spt, r.stats(), truth["spheres"][1], "the last good frame")
        torch.cuda.synchronize()
        assert_image(buf_a, truth["upbox"][0], "the frame before the rejected calls")
        assert_image(buf_b, truth["spheres"][0], "the frame behind the rejected calls")
        assert bool(torch.isnan(spare).all()), "a rejected call wrote its output"
    finally:
        closing(torch, r)


def test_rejected_late_calls_queue_nothing(spt, oracle, torch_dev, table):
    """One context, one stream, no synchronisation between the calls: a frame, a render that
    plan_launch rejects, a first-hit guide pass of another scene, a guide call its guide rejects, a
    frame of a third scene. Both frames are the oracle's, the guide holds guide_truth's records of its
    one pass (samples_done 8: the rejected guide call counted nothing). With the guide tests that put
    a pass between frames it guards the order of the one staging step both windows share
    (spt_context.cpp, stage_scene): the rejected calls rewrite the pinned staging at most after
    waiting for the upload that reads it, and the next good call restates it before its own upload."""
    import guide_truth as gt

    torch = torch_dev
    frames, truth = table
    a, b, x = frames["tilted"], frames["specular"], frames["spheres"]
    assert a.shape == (24, 32, 8)
    stream = torch.cuda.current_stream().cuda_stream
    pg = spt.default_params(width=32, height=24, spp=8, seed=15, device=0)
    cam_g = spt.Camera(aspect=a.aspect)
    want = gt.guide_truth(oracle, x.prims, cam_g._c, pg)
    late, wide = spt.spt_params.from_buffer_copy(a.p), spt.spt_params.from_buffer_copy(pg)
    for k, v in LATE_P.items():
        setattr(late, k, v)
    wide.width = 33
    r, g = spt.Renderer(0), spt.Guide(pg, 0)
    try:
        buf_a, buf_b, spare = nan_buffer(torch, a), nan_buffer(torch, b), nan_buffer(torch, a)
        enqueue(r, a, buf_a, stream)
        with pytest.raises(spt.SptError) as e:
            r.render_async(a.prims, a.cam, late, spare.data_ptr(), stream)
        assert e.value.status == 1 and str(e.value).split(": ", 1)[1] == LATE, str(e.value)
        g.render(r, x.prims, cam_g, pg, 0, 8, stream)
        with pytest.raises(spt.SptError) as e:
            g.render(r, x.prims, cam_g, wide, 0, 8, stream)
        assert e.value.status == 1, str(e.value)
        assert str(e.value).split(": ", 1)[1] == "width/height/spp differ from the guide's", str(e.value)
        assert r.kernel() == a.kernel
        enqueue(r, b, buf_b, stream)
        assert_stats(spt, r.stats(), truth["specular"][1], "frame B")
        torch.cuda.synchronize()
        assert_image(buf_a, truth["tilted"][0], "frame A")
        assert_image(buf_b, truth["specular"][0], "frame B")
        assert bool(torch.isnan(spare).all()), "the rejected render wrote its output"
        got = g.to_numpy()
        assert got.shape == want.shape and np.array_equal(got, want), \
            f"{int((got != want).sum())} guide slots differ"
        assert g.info()["samples_done"] == 8
    finally:
        closing(torch, g, r)


def window_passes(spt, fr, windows):
    """Every window through a context and a film of its own, synchronised (the construction of
    tests/test_gpu_film.py) -> [(the window's sums, the pass's statistics)]."""
    out = []
    for win in windows:
        film, r, stats, _ = film_passes(spt, fr.prims, fr.cam, fr.p, [win])
        try:
            out.append((film.to_numpy(), stats[0]))
        finally:
            film.close()
            r.close()
    return out


def test_films_and_plain_renders_share_a_context(spt, oracle, torch_dev, table):
    """One stream, no stats() until the end: the passes of a plain film (64x48 @ 16 in windows of 4,
    every other pass from a second context) and of a noise film (37x11 @ 6, batch 2) between plain
    frames of other scenes and sizes, `steal` and `big` among them.
    Bites: drop the hipMemsetAsync of c->accum (the film passes behind `steal` add its sums to
    their first three pixels); in spt_film.hip count_pass, drop `f->batches_done += 1`."""
    torch = torch_dev
    frames, truth = table
    stream = torch.cuda.current_stream().cuda_stream
    f1 = frames["head_nee"]
    f2 = fc.Frame(spt, "f2", spt.cornell_scene(), {}, dict(width=37, height=11, spp=6, seed=21), None)
    w1, w2 = [(0, 4), (4, 4), (8, 4), (12, 4)], [(0, 2), (2, 2), (4, 2)]
    ref1, ref2 = window_passes(spt, f1, w1), window_passes(spt, f2, w2)
    plain = ["spheres", "big", "steal", "upbox", "empty", "tilted"]
    A, B = spt.Renderer(0), spt.Renderer(0)
    F1, F2 = spt.Film(f1.p, 0), spt.Film(f2.p, 0)
    F2.enable_noise(2)

    def films_hold(n1, n2):
        assert F1.info() == {"width": 64, "rows": 48, "spp_total": 16, "samples_done": 4 * n1}
        assert F2.info() == {"width": 37, "rows": 11, "spp_total": 6, "samples_done": 2 * n2}
        assert F2.noise_info() == {"enabled": 1, "batch": 2, "batches_done": n2}
        assert np.array_equal(F1.to_numpy(), np.sum([s for s, _ in ref1[:n1]], axis=0, dtype=np.uint64))
        assert np.array_equal(F2.to_numpy(), np.sum([s for s, _ in ref2[:n2]], axis=0, dtype=np.uint64))
        assert np.array_equal(m2_ints(F2.noise_to_numpy()),
                              sum(s.astype(object) ** 2 for s, _ in ref2[:n2]))

    try:
        bufs, n1, n2 = [], 0, 0
        for i, k in enumerate(plain):
            # an F1 pass (contexts alternate), a plain frame, then an F2 pass while it has windows
            if n1 < 4:
                F1.render(B if n1 % 2 else A, f1.prims, f1.cam, f1.p, *w1[n1], 0, stream)
                n1 += 1
            bufs.append(nan_buffer(torch, frames[k]))
            enqueue(A, frames[k], bufs[-1], stream)
            if n2 < 3:
                F2.render(A, f2.prims, f2.cam, f2.p, *w2[n2], 0, stream)
                assert A.kernel() == "const_nee"
                n2 += 1
            if i == 1:  # the one synchronised point in the middle: two passes of each film are in
                torch.cuda.synchronize()
                films_hold(2, 2)
        assert (n1, n2) == (4, 3)
        # each context reports its own last launch: A the plain `tilted`, B the film's last window
        assert_stats(spt, A.stats(), truth["tilted"][1], "context A")
        assert A.kernel() == "const_nee_cam" and B.kernel() == "const_nee"
        assert_stats(spt, B.stats(), {k: ref1[3][1][k] for k in spt.STAT_KEYS}, "context B")
        torch.cuda.synchronize()
        films_hold(4, 3)
        assert np.array_equal(F1.resolve(), truth["head_nee"][0])
        assert np.array_equal(F2.resolve(), f2.truth(oracle)[0])
        for k, buf in zip(plain, bufs):
            assert_image(buf, truth[k][0], f"plain frame {k}")
    finally:
        closing(torch, F1, F2, A, B)


def test_an_adaptive_films_list_stays_in_its_passes(spt, torch_dev, table):
    """Two full passes of an adaptive film, a selection that retires the pixels with index % 3 == 1,
    a plain frame of another size, a listed pass, a plain frame: the plain frames are the oracle's
    and the film holds a uniform film's planes at every pixel's own count.
    Bites: launch the listed variant whenever K.pix_list was set by an earlier launch (keep
    `pix_list` in the context instead of taking it from this call's list_dev)."""
    torch = torch_dev
    frames, truth = table
    stream = torch.cuda.current_stream().cuda_stream
    fa = fc.Frame(spt, "fa", spt.cornell_scene(), {}, dict(width=33, height=14, spp=8, seed=22), None)
    U = uniform_reference(spt, fa.prims, fa.cam, fa.p, 2, 3)
    r, film = spt.Renderer(0), spt.Film(fa.p, 0)
    try:
        film.enable_noise(2)
        film.enable_adaptive()
        idx = np.arange(fa.rows * fa.width).reshape(fa.rows, fa.width)
        keep = (idx % 3 != 1).astype(np.uint8)
        film.render(r, fa.prims, fa.cam, fa.p, 0, 2, 0, stream)
        film.render(r, fa.prims, fa.cam, fa.p, 2, 2, 0, stream)
        assert film.adaptive_select(-1.0, keep, stream) == int(keep.sum())
        bufs = [nan_buffer(torch, frames[k]) for k in ("upbox", "steal", "spheres")]
        enqueue(r, frames["upbox"], bufs[0], stream)
        enqueue(r, frames["steal"], bufs[1], stream)
        film.render(r, fa.prims, fa.cam, fa.p, 4, 2, 0, stream)  # over the active list
        assert r.kernel() == "const_nee"
        assert r.stats()["samples"] == int(keep.sum()) * 2
        enqueue(r, frames["spheres"], bufs[2], stream)
        assert_stats(spt, r.stats(), truth["spheres"][1], "the plain frame behind the listed pass")
        torch.cuda.synchronize()
        for k, buf in zip(("upbox", "steal", "spheres"), bufs):
            assert_image(buf, truth[k][0], f"plain frame {k}")
        counts = film.counts_to_numpy()
        assert np.array_equal(counts, np.where(keep == 1, np.uint32(3), np.uint32(2) | RETIRED))
        sums, m2 = planes_at(U, counts & MASK)
        assert np.array_equal(film.to_numpy(), sums) and np.array_equal(film.noise_to_numpy(), m2)
        info = film.adaptive_info()
        assert (info["front"], info["n_active"]) == (3, int(keep.sum()))
        assert info["samples_total"] == 2 * 2 * keep.size + 2 * int(keep.sum())
    finally:
        closing(torch, film, r)


def test_one_context_on_two_streams(spt, torch_dev, table):
    """Order A on one context, the frames alternating between two streams, ordered by the caller
    with an event recorded after each enqueue that the other stream waits for.
    Bites: as test_pipelined_sequence (drop the accum memset; skip the scene upload when n_prims is
    unchanged). Dropping the wait for ev0 before the staging buffers are rewritten is a race that
    this test can only catch by luck."""
    torch = torch_dev
    frames, truth = table
    seq = [(k, frames[k]) for k in fc.order_a(frames)]
    r = spt.Renderer(0)
    try:
        play(spt, torch, r, seq, [torch.cuda.Stream(), torch.cuda.Stream()], False,
             truth.__getitem__)
    finally:
        closing(torch, r)


def test_two_contexts_on_two_streams(spt, torch_dev, table):
    """Two contexts on two streams at once, unordered: one plays the table top to bottom and back,
    the other bottom to top and back, each into its own buffers.
    Bites: make a per-context buffer process-wide (`static` queue, stats, d_kp or h_kp in
    spt_context)."""
    torch = torch_dev
    frames, truth = table
    labels = list(frames)
    seqs = [fc.order_a(labels), fc.order_a(labels[::-1])]
    assert seqs[0] != seqs[1] and len(seqs[0]) == len(seqs[1])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    rs = [spt.Renderer(0), spt.Renderer(0)]
    try:
        bufs = [[nan_buffer(torch, frames[k]) for k in seq] for seq in seqs]
        torch.cuda.synchronize()
        for i in range(len(seqs[0])):
            for c in (0, 1):
                enqueue(rs[c], frames[seqs[c][i]], bufs[c][i], streams[c].cuda_stream)
        for c in (0, 1):
            assert_stats(spt, rs[c].stats(), truth[seqs[c][-1]][1], f"context {c}")
        torch.cuda.synchronize()
        for c in (0, 1):
            for i, k in enumerate(seqs[c]):
                assert_image(bufs[c][i], truth[k][0], f"context {c} frame {i} ({k})")
    finally:
        closing(torch, *rs)


def test_spt_render_from_four_threads(spt, table):
    """spt.render (ctypes releases the GIL) from four threads, each on its quarter of the table,
    three rounds: every image, statistic and kernel name is the calling thread's own; one thread
    also makes a rejected call per round and reads its own error text.
    Bites: drop `thread_local` from g_dropin_kv (a thread then reads the variant of whichever
    thread rendered last) or from the error string of spt_last_error."""
    frames, truth = table
    labels = list(frames)
    failures = []
    rejected = [(dict(spp=0), "width/height/spp must be positive"),
                (dict(shard_index=7, shard_count=3), "bad shard_index/shard_count"),
                (dict(flags=0x40), "unknown flags")]

    def work(tid):
        try:
            for rnd in range(3):
                for k in labels[tid::4]:
                    fr = frames[k]
                    img, st = spt.render(fr.prims, fr.cam, fr.p, return_stats=True)
                    assert st["kernel"] == fr.kernel, (k, st["kernel"])
                    assert_stats(spt, st, truth[k][1], k)
                    assert img.shape == truth[k][0].shape and np.array_equal(
                        img.view(np.uint32), truth[k][0].view(np.uint32)), k
                if tid == 1:
                    kw, text = rejected[rnd]
                    q = spt.spt_params.from_buffer_copy(frames["head_cos"].p)
                    for key, v in kw.items():
                        setattr(q, key, v)
                    try:
                        spt.render(frames["head_cos"].prims, frames["head_cos"].cam, q)
                    except spt.SptError as e:
                        assert e.status == 1 and text in str(e), str(e)
                    else:
                        raise AssertionError(f"{kw} was not rejected")
        except BaseException as e:  # noqa: BLE001 -- handed to the main thread
            failures.append((tid, e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        spt.shutdown()
    assert not failures, failures


def test_the_callers_arrays_are_free_on_return(spt, torch_dev, table):
    """Through the C ABI directly: one prims array, one spt_camera and one spt_params, enqueued as
    `upbox`, overwritten in place with `spheres` while that frame is in flight, enqueued again.
    Both images are the oracle's of the values at call time.
    Bites: treat an equal `prims` pointer as an unchanged scene and skip to_dev / build_geo; keep
    `p` and fill the kernel parameters from it at the next call."""
    torch = torch_dev
    frames, truth = table
    lib = spt.load_library()
    a, b = frames["upbox"], frames["spheres"]
    stream = torch.cuda.current_stream().cuda_stream
    arr, cam, p = (spt.spt_prim * 64)(), spt.spt_camera(), spt.spt_params()

    def fill(fr):
        fc.scene_into(arr, fr.prims)
        ctypes.memmove(ctypes.byref(cam), ctypes.byref(fr.cam._c), ctypes.sizeof(cam))
        ctypes.memmove(ctypes.byref(p), ctypes.byref(fr.p), ctypes.sizeof(p))
        return len(fr.prims)

    r = spt.Renderer(0)
    try:
        bufs = [nan_buffer(torch, a), nan_buffer(torch, b)]
        for fr, buf in zip((a, b), bufs):
            n = fill(fr)
            assert lib.spt_render_async(r._ctx, arr, n, ctypes.byref(cam), ctypes.byref(p),
                                        ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(stream)) == 0
            assert r.kernel() == fr.kernel
        ctypes.memset(arr, 0xFF, ctypes.sizeof(arr))  # and scribbled over once both are queued
        ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
        assert_stats(spt, r.stats(), truth["spheres"][1], "the second frame")
        torch.cuda.synchronize()
        assert_image(bufs[0], truth["upbox"][0], "upbox (the arrays held spheres by then)")
        assert_image(bufs[1], truth["spheres"][0], "spheres")
    finally:
        closing(torch, r)
