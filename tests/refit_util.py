"""Shared by the vertex-update tests (hipptBvhRefit on the host, hipptUpdateVertices on the GPU): the
test scenes, the deterministic deformations, and the refit's definition restated in numpy — every
used slot's box is the float32 min/max union of the primitive boxes of the slot's subtree, each
side moved out once by pad = max(maxabs, 1e-3) * 2^-16 (one float32 operation per side, exact in
numpy), maxabs over the new primitive boxes and the extent hint."""
import copy

import numpy as np

from hippt import scenes

F = np.float32
INF = F(np.inf)


def refit_scenes():
    from test_gpu_fuzz import fuzz_scene
    return {"cornell34": scenes.cornell34, "cornell_mixed": scenes.cornell_mixed,
            "blob32x17": lambda: scenes.blob_scene(32, 17), "fuzz4": lambda: fuzz_scene(4),
            "fuzz5": lambda: fuzz_scene(5)}


def verts_of(scene) -> np.ndarray:
    return np.ascontiguousarray(scene.verts, F).reshape(-1, 9)


def extent(v0: np.ndarray) -> float:
    p = v0.reshape(-1, 3)
    return float((p.max(axis=0) - p.min(axis=0)).max())


def wobble(v0: np.ndarray, step: int = 1) -> np.ndarray:
    """V + A * sin(k * V + phase) per coordinate, A a tenth of the scene's extent."""
    e = max(extent(v0), 1e-3)
    phase = 0.7 * np.arange(9, dtype=np.float64)[None, :] + 0.37 * step
    v = v0.astype(np.float64)
    return np.ascontiguousarray(v + 0.1 * e * np.sin((7.0 / e) * v + phase), F)


def scatter(v0: np.ndarray) -> np.ndarray:
    """Every third triangle translated by twice the scene's extent: boxes must grow far."""
    v = v0.copy()
    v[::3] += F(2.0 * extent(v0))
    return np.ascontiguousarray(v, F)


def with_verts(scene, v):
    sc = copy.copy(scene)
    sc.verts = np.ascontiguousarray(v, F).reshape(np.asarray(scene.verts).shape)
    return sc


def tri_boxes(v: np.ndarray) -> np.ndarray:
    """(n, 6) lo xyz, hi xyz; a triangle with a non-finite coordinate has no box (lo +inf, hi -inf)."""
    p = v.reshape(-1, 3, 3)
    b = np.concatenate([p.min(axis=1), p.max(axis=1)], axis=1).astype(F)
    bad = ~np.isfinite(v).all(axis=1)
    b[bad, :3] = INF
    b[bad, 3:] = -INF
    return b


def sphere_boxes(spheres: np.ndarray) -> np.ndarray:
    s = np.asarray(spheres, F).reshape(-1, 4)
    r = np.abs(s[:, 3:4]) * F(1.0 + 1.0 / 4096.0)
    return np.concatenate([s[:, :3] - r, s[:, :3] + r], axis=1).astype(F)


def pad_of(boxes: np.ndarray, hint: float) -> np.float32:
    have = boxes[:, 0] <= boxes[:, 3]
    maxabs = max(F(abs(hint)), F(np.abs(boxes[have]).max()) if have.any() else F(0))
    return F(max(maxabs, F(1e-3))) * F(1.0 / 65536.0)


def slots(nodes: np.ndarray, width: int):
    """(lo [N, width, 3], hi [N, width, 3], codes [N, width] as node indices or leaf codes) of 2-wide
    (16-word) or 4-wide (32-word) nodes with node-index codes."""
    f = nodes.view(F)
    if width == 2:
        b = f[:, :12].reshape(-1, 2, 2, 3)
        return b[:, :, 0, :], b[:, :, 1, :], nodes[:, 12:14].view(np.int32)
    b = f[:, :24].reshape(-1, 3, 2, 4)  # node, axis, lo/hi, slot
    return b[:, :, 0, :].transpose(0, 2, 1), b[:, :, 1, :].transpose(0, 2, 1), nodes[:, 24:28].view(np.int32)


def check_refit(nodes: np.ndarray, width: int, pbox: np.ndarray, pad, before: np.ndarray) -> int:
    """Asserts the definition on one tree: pbox = primitive boxes in LEAF order, `before` the nodes
    of the build (codes must be unchanged, unused slots untouched).  Returns the used slots checked."""
    lo, hi, codes = slots(nodes, width)
    lo0, hi0, codes0 = slots(before, width)
    assert np.array_equal(codes, codes0), "child codes changed"
    n = len(nodes)
    # children have larger depth: resolve unions in reverse breadth-first order
    order, seen = [0], 0
    while seen < len(order):
        k = order[seen]
        seen += 1
        order.extend(int(c) for c in codes[k] if c >= 0)
    assert len(order) == n
    ulo = np.full((n, width, 3), INF, F)
    uhi = np.full((n, width, 3), -INF, F)
    checked = 0
    far = np.array([3.0e38, -1.0e20, 7.0e33], F)
    for k in reversed(order):
        for s in range(width):
            c = int(codes[k, s])
            if c < 0:
                first, count = (~c) >> 4, (~c) & 15
                if count == 0:  # unused slot: untouched
                    assert lo[k, s].tobytes() == lo0[k, s].tobytes() and hi[k, s].tobytes() == hi0[k, s].tobytes()
                    continue
                b = pbox[first:first + count]
                ulo[k, s], uhi[k, s] = b[:, :3].min(axis=0), b[:, 3:].max(axis=0)
            else:
                ulo[k, s], uhi[k, s] = ulo[c].min(axis=0), uhi[c].max(axis=0)
            if ulo[k, s, 0] <= uhi[k, s, 0]:
                elo, ehi = ulo[k, s] - pad, uhi[k, s] + pad
            else:  # every primitive below dropped: the unused slot's far point
                elo = ehi = far
            assert lo[k, s].tobytes() == elo.astype(F).tobytes(), (k, s, lo[k, s], elo)
            assert hi[k, s].tobytes() == ehi.astype(F).tobytes(), (k, s, hi[k, s], ehi)
            checked += 1
    return checked
