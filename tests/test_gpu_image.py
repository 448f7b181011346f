"""GPU image encoder (spt_image.hip) against the oracle's C restatement of the reference writer
(/root/reference/src/smallpt.cpp:313-321 toInt/clamp, :548-551 the P3 fprintf loop).

Bar: byte-identical files. P3 is also checked against the reference's own PPM (tests/golden).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FMTS = [("p3", 0), ("p6", 1), ("pfm", 2)]


def _gpu_bytes(spt, rgb, fmt):
    import torch
    h, w, _ = rgb.shape
    src = torch.from_numpy(np.ascontiguousarray(rgb, dtype=np.float32)).cuda()
    cap = spt.Encoder.bound(w, h, fmt)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    enc = spt.Encoder(0)
    try:
        n = enc.encode(src.data_ptr(), w, h, fmt, out.data_ptr(), cap)
        torch.cuda.synchronize()
    finally:
        enc.close()
    return bytes(out[:n].cpu().numpy())


def _edge_values(with_nan=True):
    f = np.float32
    thr = []
    # every toInt step of the reference formula, +-3 ulps around it (toInt is monotone)
    x = np.arange(0, 2 ** 30, 2 ** 14, dtype=np.uint32).view(np.float32)  # dense sweep of [0, 2)
    v = np.floor(np.power(np.clip(x.astype(np.float64), 0, 1), 1 / 2.2) * 255 + 0.5)
    steps = x[1:][np.diff(v) != 0]
    for s in steps:
        b = np.array([s], dtype=np.float32).view(np.uint32)[0]
        lo = max(0, int(b) - 2 ** 14)
        thr.append(np.arange(lo, int(b) + 4, dtype=np.uint32).view(np.float32))
    special = np.array([0.0, -0.0, -1.0, 1.0, 1.0000001, 2.0, 1e-45, 1e-38, np.inf, -np.inf,
                        np.nan, 0.5, 0.999999], dtype=f)
    if not with_nan:
        special = special[~np.isnan(special)]
    return np.concatenate(thr + [special])


def _edge_image(with_nan):
    vals = _edge_values(with_nan)
    n = (len(vals) + 2) // 3 * 3
    vals = np.concatenate([vals, np.zeros(n - len(vals), np.float32)])
    w = 777  # odd width, many encoder blocks with unaligned byte ranges
    h = (n // 3 + w - 1) // w
    rgb = np.zeros((h * w * 3,), np.float32)
    rgb[: len(vals)] = vals
    return rgb.reshape(h, w, 3)


@pytest.mark.parametrize("name,fmt", FMTS)
def test_encoder_matches_oracle_on_edge_values(spt, oracle, name, fmt):
    rgb = _edge_image(True)
    assert np.isnan(rgb).any()  # P3: the whole encode takes the exact slow path
    assert _gpu_bytes(spt, rgb, name) == oracle.encode_image(rgb, fmt)


@pytest.mark.parametrize("name,fmt", FMTS)
def test_encoder_matches_oracle_on_edge_values_without_nan(spt, oracle, name, fmt):
    """The same toInt steps, signed zeros, denormals and infinities without the NaN: P3 then takes
    its four-pass fast path (toInt bytes, lengths, offsets, text words), which the image with a NaN
    never enters."""
    rgb = _edge_image(False)
    assert not np.isnan(rgb).any() and np.isinf(rgb).any()
    assert _gpu_bytes(spt, rgb, name) == oracle.encode_image(rgb, fmt)


@pytest.mark.parametrize("w,h", [(1, 1), (3, 1), (1, 5), (1023, 3), (1024, 768)])
@pytest.mark.parametrize("name,fmt", FMTS)
def test_encoder_matches_oracle_sizes(spt, oracle, name, fmt, w, h):
    rgb = np.random.default_rng(w * 31 + h).random((h, w, 3), dtype=np.float32) * 1.2 - 0.1
    assert _gpu_bytes(spt, rgb, name) == oracle.encode_image(rgb, fmt)


def test_write_ppm_reproduces_reference_file(spt, oracle, tmp_path):
    """spt.write_ppm on the reference's own image == the reference's PPM (64x48@4, NEE)."""
    img = oracle.compat_render(64, 48, 4, seed=1, nee=True).astype(np.float32)
    ref = open(os.path.join(HERE, "golden", "ref_64x48_s4_nee.ppm"), "rb").read()
    assert oracle.encode_image(img, 0) == ref  # float32 framebuffer prints the same bytes here
    path = str(tmp_path / "out.ppm")
    spt.write_ppm(path, img)
    assert open(path, "rb").read() == ref


def test_rendered_image_all_formats(spt, oracle, tmp_path):
    p = spt.default_params(width=64, height=48, spp=16, seed=1)
    img = spt.render(spt.cornell_scene(), spt.Camera(aspect=64 / 48), p)
    for name, fmt in FMTS:
        path = str(tmp_path / f"r.{name}")
        spt.write_image(path, img, name)
        assert open(path, "rb").read() == oracle.encode_image(img, fmt)


def test_encode_into_too_small_buffer_fails(spt):
    import torch
    rgb = torch.zeros((4, 4, 3), dtype=torch.float32, device="cuda")
    out = torch.empty(8, dtype=torch.uint8, device="cuda")
    enc = spt.Encoder(0)
    try:
        with pytest.raises(spt.SptError):
            enc.encode(rgb.data_ptr(), 4, 4, "p3", out.data_ptr(), 8)
    finally:
        enc.close()


def test_encoder_reuse_across_nan_and_clean_images(spt, oracle):
    """P3 in passes: a NaN anywhere sends the whole encode down the exact slow path (the encode's
    epoch in the NaN word); the next encode with the same Encoder, without a NaN, takes the fast
    path again. Every output byte-identical to the oracle's writer."""
    import torch
    h, w = 200, 311  # 186,600 values: 23 text blocks, the last one partial
    rng = np.random.default_rng(7)
    clean = rng.random((h, w, 3), dtype=np.float32) * 1.2 - 0.1
    mid_nan = clean.copy()
    mid_nan[97, 150, 1] = np.nan
    last_nan = clean.copy()
    last_nan[-1, -1, -1] = np.nan
    enc = spt.Encoder(0)
    try:
        for img in (clean, mid_nan, clean, last_nan, clean):
            src = torch.from_numpy(np.ascontiguousarray(img)).cuda()
            cap = spt.Encoder.bound(w, h, "p3")
            out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            n = enc.encode(src.data_ptr(), w, h, "p3", out.data_ptr(), cap)
            torch.cuda.synchronize()
            assert bytes(out[:n].cpu().numpy()) == oracle.encode_image(img, 0)
    finally:
        enc.close()


@pytest.mark.parametrize("name,fmt", FMTS)
def test_unaligned_framebuffer_rejected_before_any_work(spt, oracle, name, fmt):
    """A framebuffer that is not 16-byte aligned is refused (SPT_ERR_INVALID_ARG) before anything is
    queued: the output buffer keeps its bytes, and the same Encoder then encodes correctly."""
    import torch
    h, w = 4, 5
    rgb = np.random.default_rng(3).random((h, w, 3), dtype=np.float32)
    buf = torch.zeros(h * w * 3 + 4, dtype=torch.float32, device="cuda")
    buf[1:1 + h * w * 3].copy_(torch.from_numpy(rgb.reshape(-1)))
    cap = spt.Encoder.bound(w, h, name)
    out = torch.full((cap,), 0xAB, dtype=torch.uint8, device="cuda")
    enc = spt.Encoder(0)
    try:
        with pytest.raises(spt.SptError, match="aligned"):
            enc.encode(buf.data_ptr() + 4, w, h, name, out.data_ptr(), cap)
        torch.cuda.synchronize()
        assert bool((out == 0xAB).all())
        src = torch.from_numpy(np.ascontiguousarray(rgb)).cuda()
        n = enc.encode(src.data_ptr(), w, h, name, out.data_ptr(), cap)
        torch.cuda.synchronize()
        assert bytes(out[:n].cpu().numpy()) == oracle.encode_image(rgb, fmt)
    finally:
        enc.close()


def _reuse_images():
    """The 311x200 images of test_encoder_reuse_across_nan_and_clean_images: 186,600 values, 23 text
    blocks, the last one partial."""
    h, w = 200, 311
    clean = np.random.default_rng(7).random((h, w, 3), dtype=np.float32) * 1.2 - 0.1
    last_nan = clean.copy()
    last_nan[-1, -1, -1] = np.nan
    return w, h, clean, last_nan


@pytest.mark.parametrize("which", ["clean", "last_nan"])
def test_p3_never_writes_at_or_past_cap(spt, oracle, which):
    """P3's length is known only after its passes, so a too small buffer is found out on the device:
    the text kernels then write the bytes below cap and nothing else (the fast path's `dst + i <
    cap`, the NaN path's `q < cap`), and the host reports the length it needed. cap around the
    header, in the middle of the text, at a 16-byte-aligned and at an odd offset inside the last text
    block, one short of the length L, and L: an error iff cap < L, naming L; every byte from cap on
    untouched; the bytes below cap the oracle's; and the same Encoder is fine afterwards."""
    import torch
    w, h, clean, last_nan = _reuse_images()
    img = clean if which == "clean" else last_nan
    want = oracle.encode_image(img, 0)
    L, hd = len(want), len(b"P3\n%d %d\n255\n" % (w, h))
    assert want[:hd] == b"P3\n311 200\n255\n"
    # where the last text block (values from 22 * 8192 on) starts in the file
    ends = hd + np.cumsum([len(t) + 1 for t in want[hd:].split(b" ")[:-1]])
    assert len(ends) == 3 * w * h and ends[-1] == L
    last0 = int(ends[22 * 8192 - 1])
    aligned = (last0 + 100) & ~15
    odd = (aligned + 33) | 1
    assert last0 < aligned < odd < L - 1 and aligned % 16 == 0 and odd % 2 == 1
    caps = [hd - 1, hd + 1, (hd + L) // 2, aligned, odd, L - 1, L]
    bound = spt.Encoder.bound(w, h, "p3")
    src = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    want_t = torch.frombuffer(bytearray(want), dtype=torch.uint8).cuda()
    enc = spt.Encoder(0)
    try:
        for cap in caps:
            out = torch.full((bound + 4096,), 0xAB, dtype=torch.uint8, device="cuda")
            if cap < L:
                with pytest.raises(spt.SptError, match=rf"need {L} bytes"):
                    enc.encode(src.data_ptr(), w, h, "p3", out.data_ptr(), cap)
            else:
                assert enc.encode(src.data_ptr(), w, h, "p3", out.data_ptr(), cap) == L
            torch.cuda.synchronize()
            assert bool((out[cap:] == 0xAB).all()), cap
            if cap >= hd:
                n = min(cap, L)
                assert torch.equal(out[:n], want_t[:n]), cap
        csrc = torch.from_numpy(np.ascontiguousarray(clean)).cuda()
        out = torch.full((bound,), 0xAB, dtype=torch.uint8, device="cuda")
        n = enc.encode(csrc.data_ptr(), w, h, "p3", out.data_ptr(), bound)
        torch.cuda.synchronize()
        assert bytes(out[:n].cpu().numpy()) == oracle.encode_image(clean, 0)
    finally:
        enc.close()


@pytest.mark.parametrize("name,fmt", [("p6", 1), ("pfm", 2)])
def test_p6_pfm_one_byte_short_is_refused_untouched(spt, oracle, name, fmt):
    """P6 and PFM know their length up front: a cap one short of it is refused before anything is
    queued, the buffer keeps every byte; cap = the length encodes."""
    import torch
    w, h, clean, _ = _reuse_images()
    want = oracle.encode_image(clean, fmt)
    L = len(want)
    src = torch.from_numpy(np.ascontiguousarray(clean)).cuda()
    out = torch.full((L + 4096,), 0xAB, dtype=torch.uint8, device="cuda")
    enc = spt.Encoder(0)
    try:
        with pytest.raises(spt.SptError, match=rf"need {L} bytes"):
            enc.encode(src.data_ptr(), w, h, name, out.data_ptr(), L - 1)
        torch.cuda.synchronize()
        assert bool((out == 0xAB).all())
        assert enc.encode(src.data_ptr(), w, h, name, out.data_ptr(), L) == L
        torch.cuda.synchronize()
        assert bytes(out[:L].cpu().numpy()) == want and bool((out[L:] == 0xAB).all())
    finally:
        enc.close()


def test_p3_more_than_8192_text_blocks(spt, oracle):
    """8190 x 2736: 67,223,520 values = 8206 text blocks of 8192, the smallest image whose block
    offsets need p3_offsets' second super-round (8192 entries per round: the carry across rounds and
    the double-buffered wave sums). One seeded random row (24,570 values, not a multiple of the
    block, so block lengths differ) repeated down the image on the device; the reference's writer
    puts no separator between rows, so the file is the header and the row's text 2736 times."""
    import time
    import torch
    w, h = 8190, 2736
    assert (3 * w * h + 8191) // 8192 == 8206
    row = np.random.default_rng(8206).random((1, w, 3), dtype=np.float32) * 1.2 - 0.1
    row_txt = oracle.encode_image(row, 0)[len(b"P3\n%d 1\n255\n" % w):]
    hd = b"P3\n%d %d\n255\n" % (w, h)
    L = len(hd) + len(row_txt) * h
    src = torch.from_numpy(row.reshape(-1)).cuda().repeat(h)
    expect = torch.cat([torch.frombuffer(bytearray(hd), dtype=torch.uint8).cuda(),
                        torch.frombuffer(bytearray(row_txt), dtype=torch.uint8).cuda().repeat(h)])
    assert expect.numel() == L and src.numel() == 3 * w * h
    out = torch.full((L + 4096,), 0xAB, dtype=torch.uint8, device="cuda")
    enc = spt.Encoder(0)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = enc.encode(src.data_ptr(), w, h, "p3", out.data_ptr(), L)
        torch.cuda.synchronize()
        print(f"8206-block P3 encode: {time.perf_counter() - t0:.3f} s, {L} bytes")
    finally:
        enc.close()
    assert n == L
    assert torch.equal(out[:L], expect)
    assert bool((out[L:] == 0xAB).all())
