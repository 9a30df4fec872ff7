"""Scenes shared by tests/test_render_pad.py (CPU model) and tests/test_gpu_render_pad.py."""
import numpy as np

from hippt import scenes

GRAZING_SIZE = (32, 32, 16)  # width, height, spp of the grazing scene's tests


def grazing_scene():
    """A floor quad and a quad tilted by 1 degree a little above it, the camera low over the floor: camera
    rays meet the floor at a few degrees, and paths bounce between two nearly parallel planes.  The oracle
    accepts self-hits among its paths (tests/test_render_pad.py asserts it)."""
    s, rise = 555.0, 555.0 * float(np.tan(np.radians(1.0)))
    floor = ((0, 0, 0), (s, 0, 0), (s, 0, s), (0, 0, s))
    lid = ((0, 30.0, 0), (0, 30.0, s), (s, 30.0 + rise, s), (s, 30.0 + rise, 0))
    tris = []
    for a, b, c, d in (floor, lid):
        tris += [a + b + c, a + c + d]
    return scenes.Scene(name="grazing", verts=np.asarray(tris, np.float64).astype(np.float32),
                        tri_mat=np.asarray([0, 0, 1, 1], np.int32),
                        albedo=np.asarray([[0.73, 0.73, 0.73], [0.65, 0.05, 0.05]], np.float32),
                        lookfrom=(278.0, 4.0, -150.0), lookat=(278.0, 6.0, 278.0))
