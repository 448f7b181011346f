"""bench.py --dump-outputs and the plain / --full split: the dump holds the image the timed path
produced (whole, or a fixed seeded sample above the size limit), and a plain run's line keeps the
headline fields while everything that takes runs of its own is left to --full."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_dump_mod", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_writes_a_small_image_whole(tmp_path):
    b = _bench()
    img = np.random.default_rng(0).random((48, 64, 3)).astype(np.float32)
    b.dump_outputs(str(tmp_path / "d"), img)
    assert os.listdir(tmp_path / "d") == ["image.npy"]
    got = np.load(tmp_path / "d" / "image.npy")
    assert got.dtype == np.float32 and np.array_equal(got, img)


def test_dump_samples_an_image_over_the_limit_the_same_way_every_time(tmp_path, monkeypatch):
    b = _bench()
    img = np.random.default_rng(1).random((48, 64, 3)).astype(np.float32)
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", img.nbytes - 1)
    b.dump_outputs(str(tmp_path / "a"), img)
    b.dump_outputs(str(tmp_path / "b"), img * 2)  # another build's image of the same size
    assert sorted(os.listdir(tmp_path / "a")) == ["image_sample.npy", "image_sample_index.npy"]
    ia, ib = (np.load(tmp_path / d / "image_sample_index.npy") for d in "ab")
    assert ia.dtype == np.float64 and np.array_equal(ia, ib)
    idx = ia.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 48 * 64
    sa, sb = (np.load(tmp_path / d / "image_sample.npy") for d in "ab")
    assert sa.dtype == np.float32 and np.array_equal(sa, img.reshape(-1, 3)[idx])
    assert np.array_equal(sb, (img * 2).reshape(-1, 3)[idx])


def test_the_4096_square_sample_fits_the_limit():
    b = _bench()
    n = min(4096 * 4096, 1 << 21)
    assert n * 3 * 4 + n * 8 <= b.DUMP_MAX_BYTES


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_image_and_leaves_the_rest_to_full(spt, tmp_path):
    """C2 at 4 spp, 3 timed steps: the dumped image is the render of those inputs bit for bit, the
    line keeps its headline fields, and nothing that needs runs of its own is in it."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "c2", "--spp", "4", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    (line,) = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert line["steps"] == 3 and line["full"] is False
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1024 * 768 * 4 / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    assert line["roofline"]["kernel_ms_source"] == "the timed launches"
    for key in ("cpu_baseline", "image_writer", "quality", "gather_equals_1gpu_render"):
        assert line[key] is None, key
    assert line["paths"]["leak_end"] is None
    assert os.listdir(out) == ["image.npy"]
    got = np.load(out / "image.npy")
    assert got.dtype == np.float32 and got.shape == (768, 1024, 3)
    p = spt.default_params(width=1024, height=768, spp=4, nee_prob=0.0, max_depth=0, tile_rows=8,
                           device=0)
    cam = spt.Camera(aspect=float(np.float32(1024) / np.float32(768)))
    assert np.array_equal(got, spt.render(spt.cornell_scene(), cam, p))
