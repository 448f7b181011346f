"""Inputs and fp64 ground truth for the contract's scalar building blocks: shared by
tests/test_contract_math.py (the oracle's C against the truth, on the CPU) and
tests/test_gpu_primitives.py (the device functions against the oracle, bit for bit).

The truth is numpy float64 / Python integers written from the formulas, never the oracle's code.
"""
import numpy as np

# Error figures of spt_device.h's comments (the project's own bounds). Two were corrected to the
# measured maximum of the exhaustive [1, 4) sweep, which is the maximum over every normal x: the
# functions commute exactly with a scaling of x by 4 (the seed's integer subtraction shifts the
# exponent by one per factor of 4 and every later operation is a mul or fma).
RCP_NR_REL = 6e-8      # measured 5.965e-8
RSQ_NR_REL = 1.33e-7   # measured 1.3242e-7; the comment said 1.3e-7 before this test existed
RSQ_NR2_REL = 5e-6     # measured 4.72e-6
RSQ_NR1_REL = 1.8e-3   # measured 1.7513e-3
# rsq_nr1 is "below the root" only up to its own roundings: where the seed is within ~1e-4 of the
# root the Newton step's 1.5 e^2 is below the three roundings that follow (h*y, the fma, the final
# mul: <= 2.5 * 2^-24 = 1.49e-7 together). Measured: at most 1.2421e-7 above the root.
RSQ_NR1_ABOVE = 1.25e-7
# The sampled direction after normalising, per component: 1e-6 with unit directions (measured
# 1.7e-7). The free-scale form takes its R = sqrt(xi2 / (1 - xi2)) from rsq_nr2, and a relative
# error eps of R turns the direction (R cos, R sin, 1) / sqrt(1 + R^2) by eps R / (1 + R^2) <=
# eps / 2: 2.36e-6 for the measured eps = 4.72e-6, on top of the unit form's error. 1e-6 cannot
# hold there; measured 2.306e-6 over all frames and both modes.
COSINE_FREE_ABS = 2.5e-6


def binade_sweep() -> np.ndarray:
    """Every float32 in [1, 4): 2^24 values, two adjacent binades (both exponent parities, which
    the rsqrt seed's shift treats differently)."""
    return np.arange(0x3F800000, 0x40800000, dtype=np.uint32).view(np.float32)


def log_uniform(n: int, lo: int, hi: int, seed: int) -> np.ndarray:
    """n float32 log-uniform in [2^lo, 2^hi)."""
    return np.exp2(np.random.default_rng(seed).uniform(lo, hi, n)).astype(np.float32)


def rel_err_rcp(x, y) -> np.ndarray:
    """y * x - 1 in float64 (the product of two floats is exact there)."""
    return np.asarray(y, np.float64) * np.asarray(x, np.float64) - 1.0


def rel_err_rsq(x, y) -> np.ndarray:
    """y * sqrt(x) - 1 in float64: positive = above the root."""
    return np.asarray(y, np.float64) * np.sqrt(np.asarray(x, np.float64)) - 1.0


SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 2.0 ** -126, 3.4028235e38, -3.4028235e38,
                     np.inf, -np.inf, np.nan], dtype=np.float32)


def disk_words() -> np.ndarray:
    """One word for each of the 2^24 values of bits 31..8 (disk_dir reads no other bit)."""
    return np.arange(1 << 24, dtype=np.uint32) << np.uint32(8)


def disk_truth(ra):
    """(cos, sin) float64 of the angle the word names: theta = u (pi/2) 2^-22 for the 21-bit
    u = bits 28..8, swapped by bit 29, signs of cos / sin = bits 31 / 30."""
    ra = np.asarray(ra, dtype=np.uint32)
    th = ((ra >> np.uint32(8)) & np.uint32(0x1FFFFF)).astype(np.float64) * (np.pi / 2 * 2.0 ** -22)
    c, s = np.cos(th), np.sin(th)
    sw = (ra & np.uint32(0x20000000)) != 0
    c, s = np.where(sw, s, c), np.where(sw, c, s)
    c = np.where((ra & np.uint32(0x80000000)) != 0, -c, c)
    s = np.where((ra & np.uint32(0x40000000)) != 0, -s, s)
    return c, s


def u01_truth(v) -> np.ndarray:
    return (np.asarray(v, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) * 2.0 ** -23


# normals for c_cosine / cosine_vec: the six axis normals, and general ones on both sides of the
# frame's |nl.x| > 0.1 branch
AXIS_NORMALS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def _unit32(v):
    v = np.asarray(v, dtype=np.float64)
    return tuple(float(x) for x in (v / np.sqrt(v @ v)).astype(np.float32))


GENERAL_NORMALS = [_unit32((0.3, -0.5, 0.8)), _unit32((0.05, 0.6, -0.79)), _unit32((-0.9, 0.1, 0.2)),
                   _unit32((0.0, 0.6, 0.8))]


def cosine_words(n: int, seed: int):
    """(ra, rb): n random word pairs, then the pairs that make a zero: the eight u = 0 azimuths
    (disk_dir's exact zeros) and xi2 = 0."""
    rng = np.random.default_rng(seed)
    ra = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    rb = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    oct8 = (np.arange(8, dtype=np.uint32) << np.uint32(29)) | np.uint32(0xA5)  # low byte: unread
    ra = np.concatenate([ra, oct8, ra[:8]])
    rb = np.concatenate([rb, rb[:8], np.arange(8, dtype=np.uint32) * np.uint32(37)])  # xi2 = 0
    return ra, rb


def cosine_truth(nl, ra, rb, uniform: bool) -> np.ndarray:
    """random_scattering in float64, normalised: the frame u = norm(|nl.x| > 0.1 ? (nl.z, 0, -nl.x)
    : (0, -nl.z, nl.y)), v = nl x u; cosine: u cos(phi) sqrt(xi2) + v sin(phi) sqrt(xi2) +
    nl sqrt(1 - xi2); uniform: radial sqrt(xi2 (2 - xi2)), normal component 1 - xi2."""
    nl = np.asarray(nl, dtype=np.float32).astype(np.float64)
    a = np.array([nl[2], 0.0, -nl[0]]) if abs(nl[0]) > 0.1 else np.array([0.0, -nl[2], nl[1]])
    u = a / np.sqrt(a @ a)
    v = np.cross(nl, u)
    c, s = disk_truth(ra)
    xi2 = u01_truth(rb)
    if uniform:
        rad, nrm = np.sqrt(xi2 * (2.0 - xi2)), 1.0 - xi2
    else:
        rad, nrm = np.sqrt(xi2), np.sqrt(1.0 - xi2)
    d = (u[None, :] * (c * rad)[:, None] + v[None, :] * (s * rad)[:, None] + nl[None, :] * nrm[:, None])
    return d / np.sqrt((d * d).sum(axis=1))[:, None]


# c_fix / fix31: (L, inv_spp) pairs
FIX_L = np.array([0.0, 1e-45, 1e-39, 1.0, 0.5, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23, 0.99999, 3.0, 1e30,
                  np.inf, np.nan, 2.0 ** -31, 2.0 ** -32, 0.3333333], dtype=np.float32)
FIX_INV_SPP = [1.0, 1.0 / 3.0, 1.0 / 16.0, 1.0 / 512.0]


def fix_pairs():
    L = np.concatenate([FIX_L, np.float32(1.0) / np.array(FIX_INV_SPP, np.float32)])  # L = spp
    inv = np.array(FIX_INV_SPP, dtype=np.float32)
    return np.tile(L, len(inv)), np.repeat(inv, len(L))


def fix_truth(L, inv_spp) -> np.ndarray:
    """floor(min(RN32(L * inv_spp), 1) * 2^31) in Python integers; NaN counts as 1 (fminf)."""
    out = []
    for a, b in zip(np.asarray(L, np.float32), np.asarray(inv_spp, np.float32)):
        v = float(np.float32(np.float64(a) * np.float64(b)))  # the exact product, rounded once
        if v != v or v >= 1.0:
            out.append(1 << 31)
        else:
            out.append(int(v * 2.0 ** 31) if v > 0.0 else 0)
    return np.array(out, dtype=np.uint32)


def makefile_hipflags(path: str) -> str:
    """The HIPFLAGS := ... assignment of a Makefile, continuation lines joined, blanks squeezed."""
    text = open(path).read().replace("\\\n", " ")
    lines = [ln for ln in text.splitlines() if ln.startswith("HIPFLAGS")]
    assert len(lines) == 1, lines
    return " ".join(lines[0].split())
