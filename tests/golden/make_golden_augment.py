"""Golden fixture of the augmentations: run the two reference functions that need no cv2 -- add_noise_to_depth
(lib/utils/augmentation.py:58-71) and the Gaussian branch of add_noise (lib/utils/blob.py:102-116,129) -- from their source on
small inputs and store the inputs, the random values and what they return.

Run in the build container only:   python tests/golden/make_golden_augment.py   ->  tests/golden/augment_reference.npz

The functions are executed from their source (_ref_import.ref_functions) in a namespace whose ``np.random`` and ``random`` are
stand-ins that hand out RECORDED values in the order the functions ask for them, so the fixture holds every number the result
depends on: the gamma variate of the depth, and for add_noise the branch variate (below 0.9: the Gaussian branch), the noise
level, the variate behind sigma and the normal field (drawn as float32 values, so that the float32 field the package takes is
the same numbers).

What could NOT be captured: chromatic_transform (cv2.cvtColor, cv2.split / merge), the motion-blur branch of add_noise
(cv2.filter2D), dropout_random_ellipses (cv2.ellipse) and add_noise_to_xyz (cv2.resize).  cv2 is not installed where this
project is built; those four are defined and tested against float64 restatements (tests/augment_cases.py) instead, and nothing
claims equality with cv2.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_import as R  # noqa: E402

NOISE_PARAMS = {"gamma_shape": 1000.0, "gamma_scale": 0.001}            # tabletop_dataset.py:37-38


class Recorded:
    """np.random / random handing out recorded values in order."""

    def __init__(self, values):
        self.values = list(values)

    def _next(self):
        return self.values.pop(0)

    def rand(self, n):
        return np.array([self._next()], dtype=np.float64)

    def randn(self, rows, cols):
        v = self._next()
        assert v.shape == (rows, cols)
        return v

    def gamma(self, shape, scale):
        return self._next()

    def uniform(self, lo, hi):
        return self._next()


def fake_numpy(rec):
    ns = types.SimpleNamespace(**{k: getattr(np, k) for k in ("clip", "repeat", "newaxis", "zeros", "ones", "float32")})
    ns.random = rec
    return ns


def main():
    rng = np.random.default_rng(41)
    out = {}
    # add_noise_to_depth
    depth = (rng.integers(0, 3000, size=(16, 20)) / 1000.0).astype(np.float32)
    depth[rng.random(depth.shape) < 0.2] = 0
    m = float(rng.gamma(NOISE_PARAMS["gamma_shape"], NOISE_PARAMS["gamma_scale"]))
    rec = Recorded([m])
    ns = R.ref_functions("lib/utils/augmentation.py", ["add_noise_to_depth"], {"np": fake_numpy(rec)})
    res = ns["add_noise_to_depth"](depth, NOISE_PARAMS)
    assert not rec.values
    out.update(depth_in=depth, depth_multiplier=np.float64(m), depth_out=np.asarray(res))
    # add_noise, Gaussian branch
    image = rng.integers(0, 256, size=(16, 20, 3), dtype=np.uint8)
    branch, level, srand = 0.5, float(rng.uniform(0, 0.1)), float(rng.random())
    field = rng.normal(size=(16, 20)).astype(np.float32)
    rec = Recorded([branch, srand, field.astype(np.float64)])
    ns = R.ref_functions("lib/utils/blob.py", ["add_noise"], {"np": fake_numpy(rec), "random": Recorded([level])})
    res = ns["add_noise"](image)
    assert not rec.values and res.dtype == np.uint8
    out.update(noise_in=image, noise_branch=np.float64(branch), noise_level=np.float64(level), noise_rand=np.float64(srand),
               noise_sigma=np.float64(srand * level * 256), noise_field=field, noise_out=res)
    path = os.path.join(HERE, "augment_reference.npz")
    np.savez_compressed(path, **out)
    print(f"augment_reference: multiplier {m:.6f}, sigma {srand * level * 256:.4f}, {(res != image).mean() * 100:.1f} % of the bytes changed, "
          f"{os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
