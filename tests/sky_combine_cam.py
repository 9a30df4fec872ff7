"""The camera of the HIPPT_OPT_SKY_COMBINE tests: cornell34's pinhole pulled back along its axis until the
room covers the middle third of a 104x72 image, so that whole 8x8 sky tiles lie on all four sides of the
sky rectangle (tests/test_sky_combine_model.py asserts it with the product's own sky_rect();
tests/test_gpu_sky_combine.py renders with it)."""
import dataclasses

import numpy as np

from hippt import scenes

WIDTH, HEIGHT = 104, 72
PULLED_BACK = dict(lookfrom=(278.0, 278.0, -2400.0))


def pulled_back(make=scenes.cornell34, **more):
    return dataclasses.replace(make(), **PULLED_BACK, **more)


def root_box(sc):
    """cornell34's root box as the builder pads it, and the pad (tests/test_gpu_sky_rect.py's restatement)."""
    p = np.ascontiguousarray(sc.verts, np.float32).reshape(-1, 3)
    m = np.float32(max(float(np.abs(p).max()), max(abs(c) for c in sc.lookfrom)))
    pad = np.float32(m * np.float32(2.0 ** -16))
    return (p.min(axis=0) - pad).astype(np.float32), (p.max(axis=0) + pad).astype(np.float32), pad
