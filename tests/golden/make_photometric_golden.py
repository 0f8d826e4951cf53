#!/usr/bin/env python3
"""Record tests/golden/photometric.npz by running the REFERENCE's photometric functions.

Run where the reference tree is available (it never travels to the GPU machine):

    python tests/golden/make_photometric_golden.py [path of the reference's balf/datasets/dataset_utils.py]

balf/datasets/dataset_utils.py imports cv2 and imgaug (absent offline), so bgr_distorsion, check_margins, swap_channels and
bgr_photometric_to_rgb are compiled from the reference's source with ``ast`` and run unchanged, as make_pair_synth_golden.py
does, and ``perms`` is read from the same source.  What is NOT the reference's: ``cv2.cvtColor`` is
tests/photometric_common.py's restatement of OpenCV's scalar 8-bit conversions, so the fixture pins the reference's OWN
statements -- the order and the arguments of its draws, the float64 clamps, the truncating casts, the hue wrap, the channel
swap -- around conversions that include/balf_hip.h defines; parity with a cv2 build stays unpinned.

The functions see ``np`` through a proxy whose ``random`` logs every call, so the recorded draws are the reference's, not the
port's.  Per seed s of SEEDS, after ``np.random.seed(s)``:
  draws.s.log     float64 [n,4]: per call (0 = randint / 1 = uniform, first argument, second argument or nan, the value)
  draws.s.state   the generator's 624 words and position after the call
  draws.s.params  float64 [6]: (delta_b, alpha1, sat, hue, alpha2, perm) read off the log (a branch that did not fire: neutral)
  draws.s.fired   the five coins (brightness, contrast, saturation, hue, swap)
  img.s.k.in/out  the k-th 16 x 16 BGR image (photometric_common.fixture_image) and bgr_distorsion of it, every image after its
                  own np.random.seed(s); rgb.s = bgr_photometric_to_rgb of image 0
and once: perms, and cast_u8 = np.array([324.5, 359.9, 255.9]).astype(np.uint8), the cast the hue wrap relies on.

Asserted here: every coin falls both ways, alone and in each pair with another coin (all 32 combinations of five coins cannot
be expected of 32 seeds; the steps interact pairwise at most: brightness with hue through ``delta``, contrast with itself);
the hue wrap occurs in both directions (x < 0 -> + 360, which the cast then folds to 68..103; x >= 180, past hrange, which
HSV2RGB_b brings back by subtracting 6 -- x > 360 cannot occur: H < 180 and |hue| <= 36); the restatement with the
read-off parameters gives the reference's output."""
import ast
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

from tests.golden.make_golden import ref_functions                  # noqa: E402
from tests import photometric_common as PC                          # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/balf/datasets/dataset_utils.py"
FUNCS = ["bgr_distorsion", "check_margins", "swap_channels", "bgr_photometric_to_rgb"]


class LoggedRandom:
    """np.random with a log of (kind, a, b, value) rows."""

    def __init__(self):
        self.log = []

    def randint(self, *a):
        v = np.random.randint(*a)
        self.log.append((0.0, float(a[0]), float(a[1]) if len(a) > 1 else np.nan, float(v)))
        return v

    def uniform(self, lo, hi):
        v = np.random.uniform(lo, hi)
        self.log.append((1.0, float(lo), float(hi), float(v)))
        return v


class NumpyProxy:
    def __init__(self, random):
        self.random = random

    def __getattr__(self, name):
        return getattr(np, name)


def reference_perms():
    for node in ast.parse(open(REF).read()).body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "perms":
            return ast.literal_eval(node.value)
    raise AssertionError("perms not found")


def read_off(log):
    """The reference's call log -> ((delta_b, alpha1, sat, hue, alpha2, perm), the five coins)."""
    it = iter(log)

    def coin():
        kind, a, b, v = next(it)
        assert kind == 0 and a == 2 and np.isnan(b)
        return int(v)

    def uniform():
        kind, a, b, v = next(it)
        assert kind == 1
        return v

    bright = coin()
    delta_b = uniform() if bright else 0.0
    contrast = coin()
    alpha1 = uniform() if contrast else 1.0
    sat_on = coin()
    sat = uniform() if sat_on else 1.0
    hue_on = coin()
    hue = uniform() if hue_on else 0.0
    alpha2 = uniform() if contrast else 1.0
    swap = coin()
    perm = 0
    if swap:
        kind, a, b, perm = next(it)
        assert kind == 0 and a == 6
    assert next(it, None) is None
    return (delta_b, alpha1, sat, hue, alpha2, float(perm)), (bright, contrast, sat_on, hue_on, swap)


def main():
    perms = reference_perms()
    assert tuple(perms) == PC.PERMS
    fx = {"meta.seeds": np.asarray(PC.SEEDS), "meta.images_per_seed": PC.IMAGES_PER_SEED, "perms": np.asarray(perms),
          "cast_u8": np.array([324.5, 359.9, 255.9]).astype(np.uint8)}
    coins, wraps = [], set()
    for s in PC.SEEDS:
        for k in range(PC.IMAGES_PER_SEED):
            rnd = LoggedRandom()
            ref = ref_functions(REF, FUNCS, {"np": NumpyProxy(rnd), "cv2": PC.CV2_STUB, "perms": perms})
            im = PC.fixture_image(s, k)
            np.random.seed(s)
            out = ref["bgr_distorsion"](im.copy())
            state = np.random.get_state()
            log = np.asarray(rnd.log, np.float64)
            params, fired = read_off(rnd.log)
            assert out.dtype == np.uint8 and out.shape == im.shape
            if k == 0:
                fx[f"draws.{s}.log"], fx[f"draws.{s}.params"], fx[f"draws.{s}.fired"] = log, np.asarray(params), np.asarray(fired)
                fx[f"draws.{s}.state"] = np.append(state[1], state[2]).astype(np.uint32)
                coins.append(fired)
                np.random.seed(s)
                rgb = ref["bgr_photometric_to_rgb"](im.copy())
                assert np.array_equal(rgb, out[:, :, ::-1])
                fx[f"rgb.{s}"] = rgb
            else:
                assert np.array_equal(log, fx[f"draws.{s}.log"], equal_nan=True)
            fx[f"img.{s}.{k}.in"], fx[f"img.{s}.{k}.out"] = im, out
            p, perm = PC.draws_to_params(params)
            assert np.array_equal(PC.distort(im, p, perm), out), (s, k)
            # the hue wrap, on the values the reference forms
            pre = np.clip(np.clip(im.astype(float) + p[0], 0, 255) * p[1], 0, 255).astype(np.uint8)
            x = PC.bgr2hsv_u8(pre)[..., 0].astype(float) + p[3]
            if (x < 0).any():
                wraps.add("below")
            if (x >= 180).any():
                wraps.add("above")
    coins = np.asarray(coins)
    for i in range(5):
        for j in range(5):
            for a in (0, 1):
                for b in (0, 1):
                    assert ((coins[:, i] == a) & (coins[:, j] == b)).any() or (i == j and a != b), (i, j, a, b)
    assert wraps == {"below", "above"}, wraps
    assert list(fx["cast_u8"]) == [68, 103, 255], fx["cast_u8"]
    print("combinations of the five coins among the seeds:", len({tuple(c) for c in coins}), "of 32")
    out = os.path.join(HERE, "photometric.npz")
    np.savez_compressed(out, **fx)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
