"""Shared by the photometric tests (test_photometric_host.py, test_photometric_gpu.py) and the recording script
(tests/golden/make_photometric_golden.py): access to tests/golden/photometric.npz and a NumPy restatement of the distortion
that include/balf_hip.h DEFINES (balf_photometric_u8, balf_synth_train_pairs): the reference's bgr_distorsion with the two
cv2 colour conversions written out after OpenCV's scalar 8-bit code.  Parity with a cv2 build is unpinned; the
reference's own statements around the conversions ARE pinned, by the fixture."""
import functools
import os
import types

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photometric.npz")
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
NEUTRAL = (0.0, 1.0, 1.0, 0.0, 1.0)         # (delta_b, alpha1, sat, hue, alpha2): every step the identity
SEEDS = tuple(range(32))
IMAGES_PER_SEED = 2                         # 16 x 16 images recorded per seed
COLOR_BGR2HSV, COLOR_HSV2BGR, COLOR_BGR2RGB = "BGR2HSV", "HSV2BGR", "BGR2RGB"


def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def fixture_image(seed, k):
    """The k-th 16 x 16 BGR test image of a seed: random bytes with gray, saturated and tied-channel pixels planted."""
    rng = np.random.default_rng(9000 + 10 * seed + k)
    im = rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)
    im[0, :, :] = rng.integers(0, 256, (16, 1), dtype=np.uint8)                  # gray: S == 0
    im[1, :, 1] = im[1, :, 0]                                                    # b == g
    im[2, :, 2] = im[2, :, 1]                                                    # g == r
    im[3, :, 2] = im[3, :, 0]                                                    # b == r
    im[4, :8] = (0, 0, 255)
    im[4, 8:] = (255, 0, 0)
    im[5, :4], im[5, 4:8], im[5, 8:12], im[5, 12:] = (0, 0, 0), (255, 255, 255), (0, 255, 0), (255, 0, 255)
    return im


# ---- OpenCV's scalar 8-bit conversions --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def div_tables():
    i = np.arange(256, dtype=np.float64)
    with np.errstate(divide="ignore"):
        sdiv = np.rint((255 << 12) / i)
        hdiv = np.rint((180 << 12) / (6.0 * i))
    sdiv[0] = hdiv[0] = 0
    return sdiv.astype(np.int32), hdiv.astype(np.int32)


def bgr2hsv_u8(bgr):
    """RGB2HSV_b, hrange 180: uint8 [...,3] (b, g, r) -> uint8 [...,3] (h, s, v)."""
    sdiv, hdiv = div_tables()
    b, g, r = (bgr[..., k].astype(np.int32) for k in range(3))             # (|h * hdiv| < 2^31: int32 as in OpenCV)
    v, vmin = np.maximum(np.maximum(b, g), r), np.minimum(np.minimum(b, g), r)
    diff = v - vmin
    s = (diff * sdiv[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + 2048) >> 12                               # (NumPy's >> on a negative integer is arithmetic)
    h = h + np.where(h < 0, 180, 0)
    assert s.max(initial=0) <= 255 and h.min(initial=0) >= 0 and h.max(initial=0) < 180
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


_SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


def hsv2bgr_u8(hsv):
    """HSV2RGB_b through its float32 path, no fused operations: uint8 [...,3] (h, s, v) -> uint8 [...,3] (b, g, r)."""
    f32 = np.float32
    inv255 = f32(1.0) / f32(255.0)
    hb, sb, vb = (hsv[..., k] for k in range(3))
    s, vv = sb.astype(f32) * inv255, vb.astype(f32) * inv255
    hh = hb.astype(f32) * (f32(6.0) / f32(180.0))
    hh = np.where(hh >= f32(6.0), hh - f32(6.0), hh).astype(f32)
    sector = np.floor(hh).astype(np.int8)
    f = (hh - sector.astype(f32)).astype(f32)
    assert sector.min(initial=0) >= 0 and sector.max(initial=0) <= 5
    one = f32(1.0)
    tab = [vv, vv * (one - s), vv * (one - s * f), vv * (one - s * (one - f))]
    gray = sb == 0
    out = np.empty(hsv.shape, np.uint8)
    for k in range(3):
        x = np.choose(_SECTOR[:, k][sector], tab)
        x = np.where(gray, vv, x).astype(f32)
        out[..., k] = np.clip(np.rint(x * f32(255.0)), 0, 255)                    # rint: half to even
    return out


def cvt_color(img, code):
    """What stands in for cv2.cvtColor when the reference's functions are run by the recorder."""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3, (img.dtype, img.shape)
    if code == COLOR_BGR2HSV:
        return bgr2hsv_u8(img)
    if code == COLOR_HSV2BGR:
        return hsv2bgr_u8(img)
    assert code == COLOR_BGR2RGB, code
    return np.ascontiguousarray(img[..., ::-1])


CV2_STUB = types.SimpleNamespace(cvtColor=cvt_color, COLOR_BGR2HSV=COLOR_BGR2HSV, COLOR_HSV2BGR=COLOR_HSV2BGR,
                                 COLOR_BGR2RGB=COLOR_BGR2RGB)


# ---- the seven steps of include/balf_hip.h ----------------------------------------------------------------------------------
def _clamp(x):
    x = np.array(x, dtype=np.float64)
    x[x > 255.0] = 255.0
    x[x < 0.0] = 0.0
    return x


_BYTES = np.arange(256, dtype=np.float64)


def distort(img, params, perm, blue_idx=0):
    """uint8 [...,3] in B, G, R order (``blue_idx`` 0) or R, G, B (2) -> the distorted image in the same order; ``params`` =
    (delta_b, alpha1, sat, hue, alpha2), ``perm`` a row of PERMS.  Steps 1, 3, 4 and 6 act on one byte at a time: their
    float64 expressions are evaluated at the 256 bytes and looked up, which is the same function of every pixel (the recorder
    checks the result against the reference's whole-array arithmetic) and keeps the 2^24-pixel case quick."""
    delta_b, alpha1, sat, hue, alpha2 = (float(v) for v in params)
    img = np.asarray(img)
    bgr = img if blue_idx == 0 else img[..., ::-1]
    x = _clamp(_clamp(_BYTES + delta_b) * alpha1).astype(np.uint8)[bgr]                           # 1
    hsv = bgr2hsv_u8(x)                                                                           # 2
    s = _clamp(_BYTES * sat).astype(np.uint8)[hsv[..., 1]]                                        # 3
    h = _BYTES + hue                                                                              # 4
    h = np.where(h > 360.0, h - 360.0, h)
    h = np.where(h < 0.0, h + 360.0, h)
    h = (h.astype(np.int32) & 255).astype(np.uint8)[hsv[..., 0]]    # truncation toward zero, then the low byte
    x = hsv2bgr_u8(np.stack([h, s, hsv[..., 2]], axis=-1))                                        # 5
    x = _clamp(_BYTES * alpha2).astype(np.uint8)[x]                                               # 6
    x = x[..., list(PERMS[perm])]                                                                 # 7
    return np.ascontiguousarray(x if blue_idx == 0 else x[..., ::-1])


def draws_to_params(d):
    """A recorded row of draws (see make_photometric_golden.py: DRAW_FIELDS) -> (params [5], perm)."""
    return np.asarray(d[:5], np.float64), int(d[5])
