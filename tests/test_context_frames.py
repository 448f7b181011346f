"""The frame table of tests/frame_cases.py, checked on the CPU with the oracle and spt_select_kernel
alone, so that tests/test_gpu_context_frames.py cannot pass vacuously: the frames reach the kernels
the table names, consecutive frames of both orders differ in the launch and in the image (a frame
that wrongly kept its predecessor's state cannot pass by coincidence), the orders grow and shrink
every buffer, and every link of the one-input chain changes the image."""
import pytest

import frame_cases as fc


@pytest.fixture(scope="module")
def table(spt, oracle):
    frames = fc.frames(spt)
    return frames, {k: f.truth(oracle) for k, f in frames.items()}


def test_the_table_names_the_issues_frames(spt, table):
    import test_gpu_film
    import test_gpu_parity
    frames, _ = table
    assert list(frames) == ["head_nee", "head_cos", "tilted", "upbox", "nobox", "uplight", "spheres",
                            "specular", "uniform", "leaks", "steal", "shard", "empty", "big"]
    assert {k: f.shape for k, f in frames.items()} == {
        "head_nee": (48, 64, 16), "head_cos": (30, 40, 8), "tilted": (24, 32, 8),
        "upbox": (17, 33, 12), "nobox": (12, 16, 2), "uplight": (18, 24, 6), "spheres": (18, 24, 4),
        "specular": (24, 32, 12), "uniform": (9, 17, 5), "leaks": (30, 40, 8), "steal": (1, 3, 2048),
        "shard": (16, 64, 6), "empty": (0, 16, 2), "big": (72, 96, 4)}
    assert frames["head_nee"].p.seed == 1
    assert fc.TILTED is test_gpu_film.TILTED and frames["tilted"].camkw == test_gpu_film.TILTED
    assert frames["uplight"].kernel == test_gpu_parity.EDITS_LR_AUTO[0]
    assert max(f.n_values for f in frames.values()) == frames["big"].n_values


def test_every_frame_selects_the_tables_kernel(spt, table):
    frames, _ = table
    seen = set()
    for k, f in frames.items():
        if f.rows == 0:
            assert f.kernel is None, k
            continue
        assert spt.select_kernel(f.prims, f.cam, f.p)["name"] == f.kernel, k
        seen.add(f.kernel)
    assert {"const_nee", "const_cos", "const_nee_cam", "upbox_nee", "rectdiff_nee", "uplight_nee",
            "sphdiff_nee", "generic", "const_nee_ref"} <= seen
    assert len(seen) >= 9 and sum(f.rows == 0 for f in frames.values()) == 1


def test_every_image_has_light_and_shade(table):
    frames, truth = table
    for k, f in frames.items():
        img, st = truth[k]
        assert img.shape == (f.rows, f.width, 3), k
        if f.rows == 0:
            assert not any(st.values()), k
            continue
        assert (img != 0).any() and (img < 1).any(), k
        assert st["samples"] == f.rows * f.width * f.spp, k


@pytest.mark.parametrize("order", ["A", "B"])
def test_consecutive_frames_differ(table, order):
    """... in the kernel or the launch's sizes, and in at least 1 % of the image's values (on the
    overlapping prefix; next to `empty` there are no values to compare, and the kernel differs)."""
    frames, truth = table
    seq = fc.ORDERS[order](frames)
    assert len(seq) >= 2 * len(frames) - 1 and set(seq) == set(frames)
    for a, b in zip(seq, seq[1:]):
        fa, fb = frames[a], frames[b]
        assert fa.kernel != fb.kernel or fa.shape != fb.shape, (a, b)
        frac = fc.fraction_differing(truth[a][0], truth[b][0])
        if frac is None:
            assert "empty" in (a, b) and fa.kernel != fb.kernel, (a, b)
        else:
            assert frac >= 0.01, (a, b, frac)


def test_order_a_grows_and_shrinks(table):
    frames, _ = table
    seq = fc.order_a(frames)
    assert seq[:len(frames)] == list(frames) and seq[len(frames) - 1:] == list(frames)[::-1]
    for size in (lambda f: f.rows * f.width, lambda f: f.n_units()):
        steps = [size(frames[b]) - size(frames[a]) for a, b in zip(seq, seq[1:])]
        assert max(steps) > 0 > min(steps)
    # every frame but the two ends of the table follows two different predecessors
    before = {}
    for a, b in zip(seq, seq[1:]):
        before.setdefault(b, set()).add(a)
    assert all(len(before[k]) == 2 for k in list(frames)[1:-1])


def test_order_b_second_round_grows_nothing(table):
    frames, _ = table
    seq = fc.order_b(frames)
    n = len(frames)
    assert len(seq) == 2 * n and sorted(seq[:n]) == sorted(seq[n:]) == sorted(frames)
    assert seq[n] == "big" and seq[:n] != list(frames)


def test_every_link_of_the_chain_changes_the_image(spt, oracle):
    links = fc.chain(spt)
    assert fc.N_LINKS >= 14 and len(links) == 1 + fc.N_LINKS + 2
    names = [what for what, _ in links]
    assert names[0] == "first" and names[-2:] == ["first_again", "first_again_2"]
    for must in ("seed", "nee_prob", "rr_depth", "max_depth", "light_e", "wall_c", "lookat",
                 "box_moved", "light_edited", "flags_uniform", "flags_leaks", "flags_generic", "spp",
                 "width", "height"):
        assert must in names, must
    first = links[0][1]
    assert first.shape == (24, 32, 8) and first.kernel == "const_nee"
    assert links[-1][1] is first and links[-2][1] is first
    imgs = [f.truth(oracle)[0] for _, f in links]
    for k in range(1, len(links) - 1):  # the last pair is the same frame twice, on purpose
        frac = fc.fraction_differing(imgs[k - 1], imgs[k])
        assert frac is not None and frac >= 0.01, (names[k], frac)
    # the links reach kernels of every level, not one
    assert len({f.kernel for _, f in links}) >= 4
