#!/usr/bin/env python3
"""Generate tests/golden/image_io.npz: three resize cases pinned as data -- the seeded uint8 input, Pillow's own
``Image.resize`` output, and the integer tables (``bounds``, ``kk`` per axis) that reproduce it.

The outputs come from Pillow (whatever version runs this script; 12.2 when the fixture was written).  The tables come from
``pd_resample_coefficients`` and are stored only after the integer two-pass of tests/image_ref.py, fed with them, has
reproduced Pillow's bytes exactly -- so the fixture pins both the tables and the pixels, whatever Pillow a later test run finds.

Cases (keys prefixed by the tag): H x W -> H x W, filter
  up     37 x 53   -> 64 x 64   lanczos
  down   64 x 64   -> 37 x 53   box
  check  129 x 200 -> 64 x 64   lanczos, on the 0 / 255 checkerboard (the clip matters)
Keys: <tag>_in, <tag>_out, <tag>_bounds_h, <tag>_kk_h (the horizontal pass: Ws -> W), <tag>_bounds_v, <tag>_kk_v (Hs -> H).

Usage: python tests/golden/make_golden_image_io.py   (needs the built library, Pillow and NumPy)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from prompt_diffusion_amd import engine as E  # noqa: E402
from tests import image_ref as R  # noqa: E402

CASES = (("up", (37, 53), (64, 64), "lanczos"), ("down", (64, 64), (37, 53), "box"), ("check", (129, 200), (64, 64), "lanczos"))


def main():
    out = {}
    for tag, src, dst, filt in CASES:
        img = R.seeded_image(src, seed=11)
        ref = R.pil_resize(img, dst, filt)
        assert np.array_equal(R.resize_u8(img, dst, E.resample_coefficients, filt), ref), tag
        bh, kh = E.resample_coefficients(src[1], dst[1], filt)
        bv, kv = E.resample_coefficients(src[0], dst[0], filt)
        out.update({f"{tag}_in": img, f"{tag}_out": ref, f"{tag}_bounds_h": bh, f"{tag}_kk_h": kh, f"{tag}_bounds_v": bv,
                    f"{tag}_kk_v": kv})
    path = os.path.join(HERE, "image_io.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
