"""The reference of light selection by power (include/hippt.h HIPPT_OPT_LIGHT_SELECT HIPPT_LIGHT_SELECT_POWER,
DESIGN.md §18): the selection table in numpy integers and float32, and nee_ref.NeeRef / mis_ref.MisRef with the
selection draw and the factor float32(nLights) replaced.  This file is the statement of record of the rule; the GPU
matches the table word for word and the paths bit for bit.

The lights j = 0 .. n-1 are the emissive primitives in ascending id.  Every float operation is one float32
operation in the association written; everything summed is an integer.

  A_j    the light's area as the connection forms it: a triangle's 0.5 * sqrt(fdot(c, c)), c = fcross(e1, e2), from
         the primitive record's edges e1 = v1 - v0, e2 = v2 - v0 (a record whose |c| is not above 0 holds zero
         edges, so A_j = 0); a sphere's (12.566371 * r) * r
  y_j    (Le.r + Le.g) + Le.b of its material
  lit_j  A_j > 0 and y_j > 0 (false for NaN);   W_j = A_j * y_j if lit_j else 0
  Wmax   max_j W_j;   flat = not (Wmax > 0 and Wmax < +inf)
  q_j    not lit_j: 0;   flat: 1;   else min(4096, max(1, int((W_j / Wmax) * 4096)))     (uint32)
  c_j    q_0 + ... + q_j (uint32);   T = c_{n-1}
  ip_j   float32(T) / float32(q_j) if q_j > 0 else 0

  selection draw   rng = hash32(rng) (po_rand01 advances the state exactly so); x = (rng * T) >> 32 in 64 bits.
                   T == 0: no shadow ray and no further draw.  Else k = the light with the smallest j, c_j > x.
  connection       NeeRef's / MisRef's with ip_k in place of float32(nLights)
  MIS light hit    MisRef's with the hit light's ip in place of float32(nLights); q == 0 gives wb = 1

The table takes effect for n <= LIGHT_MAX lights (T < 2^32); above that the paths are the uniform rule's."""
import ctypes
import functools

import numpy as np

import hippt
import mis_ref as mr
import nee_ref as nr
import path_ref as pr
import pyoracle as po
from hit_ref import fcross, fdot, fmaf
from hippt import scenes
from nee_ref import BACKFACING, FAR_SIDE, PI, F, INF
from mis_ref import INFINITE_G

LIGHT_MAX = (1 << 20) - 1
Q_ONE = 4096
DTYPE = hippt.LIGHT_TABLE_DTYPE

# further event bits (detail["events"]) beside nee_ref's and mis_ref's
FLOOR_SELECTED = 1024   # the selected light's q is the floor, 1, in a table that is not flat
NO_LIGHT = 2048         # T == 0: no light could be selected
EVENTS = dict(mr.EVENTS, **{"floor selected": FLOOR_SELECTED, "no light": NO_LIGHT})


def light_ids(sc):
    """The emissive primitives of a scene in ascending id (triangles, then spheres)."""
    m = sc.materials()
    kind = np.concatenate([m["kind"][np.asarray(sc.tri_mat, np.int64)], m["kind"][np.asarray(sc.sph_mat, np.int64)]])
    return np.flatnonzero(kind == scenes.MAT_EMISSIVE).astype(np.int64)


def light_area(sc, k):
    """A_k of primitive k of the scene, from the vertices as the upload forms the record's edges."""
    nt = sc.num_tris
    if k >= nt:
        r = F(np.asarray(sc.spheres, F).reshape(-1, 4)[k - nt][3])
        return (nr.FOUR_PI * r) * r
    v = np.asarray(sc.verts, F)[k]
    e1 = tuple(F(v[3 + i]) - F(v[i]) for i in range(3))
    e2 = tuple(F(v[6 + i]) - F(v[i]) for i in range(3))
    c = fcross(e1, e2)
    root = np.sqrt(fdot(c, c))
    return F(0.5) * root if root > 0 else F(0.0)  # (not above 0: the record's edges are zeroed)


def from_weights(prim, area, y):
    """The table of lights with ids `prim`, areas `area` and emission sums `y` (float32 arrays)."""
    n = len(prim)
    tab = np.zeros(n, DTYPE)
    tab["prim"] = prim
    if n == 0:
        return tab
    area, y = np.asarray(area, F), np.asarray(y, F)
    with np.errstate(all="ignore"):
        lit = (area > 0) & (y > 0)
        w = np.where(lit, area * y, F(0.0)).astype(F)
        wmax = F(w.max())
        flat = not (wmax > 0 and wmax < INF)
        if flat:
            q = lit.astype(np.uint32)
        else:
            r = ((w / wmax) * F(Q_ONE)).astype(F)
            q = np.where(lit, np.minimum(Q_ONE, np.maximum(1, r.astype(np.int64))), 0).astype(np.uint32)
        c = np.cumsum(q.astype(np.uint64))
        assert int(c[-1]) < 1 << 32
        total = F(int(c[-1]))
        ip = np.where(q > 0, total / np.maximum(q, 1).astype(F), F(0.0)).astype(F)
    tab["q"], tab["c"], tab["ip"] = q, c.astype(np.uint32), ip
    return tab


def table(sc):
    """The selection table of a scene: a structured array (prim, q, c, ip), one entry per light in ascending id."""
    ids = light_ids(sc)
    m = sc.materials()
    mat = np.concatenate([np.asarray(sc.tri_mat, np.int64), np.asarray(sc.sph_mat, np.int64)])[ids]
    le = m["albedo"][mat].astype(F).reshape(-1, 3)
    y = (le[:, 0] + le[:, 1]) + le[:, 2]
    area = np.array([light_area(sc, int(k)) for k in ids], F)
    return from_weights(ids, area, y)


def select(tab, rng_word):
    """The index j of the light the hashed RNG word selects in a table with T > 0."""
    x = (int(rng_word) * int(tab["c"][-1])) >> 32
    return int(np.searchsorted(tab["c"], x, side="right"))


class _Select:
    """What both references share: the table, the selection draw and ip."""

    def init_table(self, sc):
        self.tab = table(sc)
        assert [int(p) for p in self.tab["prim"]] == self.lights
        self.use_table = 0 < len(self.lights) <= LIGHT_MAX
        self.ip_of = {int(p): F(v) for p, v in zip(self.tab["prim"], self.tab["ip"])}
        self.q_of = {int(p): int(v) for p, v in zip(self.tab["prim"], self.tab["q"])}
        self.floor_matters = bool(len(self.tab)) and int(self.tab["q"].max()) > 1

    def pick(self, st):
        """(light id or None when T == 0, ip) from RNG state st (advanced by one draw)."""
        po.lib().po_rand01(ctypes.byref(st))
        if int(self.tab["c"][-1]) == 0:
            return None, F(0.0)
        j = select(self.tab, st.value)
        return int(self.tab["prim"][j]), F(self.tab["ip"][j])

    def geometry(self, k, p, n, st):
        """NeeRef.connect's geometry for light k: (om, cosS, cosL, d2, A, why)."""
        q, nl, A, sph = self.light_point(k, st)
        w = tuple(q[i] - p[i] for i in range(3))
        d2 = fdot(w, w)
        il = F(1.0) / np.sqrt(d2)
        om = tuple(w[i] * il for i in range(3))
        cos_s = fdot(n, om)
        s_l = fdot(nl, om)
        why = 0
        if sph is None:
            cos_l = np.abs(s_l)
        else:
            c, r = sph
            oc = tuple(p[i] - c[i] for i in range(3))
            outside = bool(fdot(oc, oc) >= r * r)
            cos_l = -s_l if outside else s_l
            if outside and not cos_l > 0:
                why = FAR_SIDE
        if not cos_s > 0:
            why = BACKFACING
        return om, cos_s, cos_l, d2, A, why

    def connect_select(self, p, n, thr, st, mis):
        k, ip = self.pick(st)
        if k is None:
            return None, (F(0.0), F(0.0), F(0.0)), -1, NO_LIGHT
        note = FLOOR_SELECTED if self.floor_matters and self.q_of[k] == 1 else 0
        om, cos_s, cos_l, d2, A, why = self.geometry(k, p, n, st)
        if not cos_s > 0 or not cos_l > 0 or not d2 > 0 or not A > 0:
            return None, om, k, why | note
        g = (((cos_s * cos_l) * A) * ip) / (PI * d2)
        if mis:
            if not g < INF:
                return None, om, k, INFINITE_G | note
            g = g / fmaf(g, g, F(1.0))
        le = self.prim_emission[k]
        return tuple((F(thr[i]) * le[i]) * g for i in range(3)), om, k, note


class SelectNeeRef(_Select, nr.NeeRef):
    """nee_ref.NeeRef under HIPPT_LIGHT_SELECT_POWER."""

    def __init__(self, sc, ref, sample=True):
        nr.NeeRef.__init__(self, sc, ref, sample)
        self.init_table(sc)

    def connect(self, p, n, thr, st):
        if not self.use_table:
            return nr.NeeRef.connect(self, p, n, thr, st)
        return self.connect_select(p, n, thr, st, False)


class SelectMisRef(_Select, mr.MisRef):
    """mis_ref.MisRef under HIPPT_LIGHT_SELECT_POWER."""

    def __init__(self, sc, ref, sample=True):
        mr.MisRef.__init__(self, sc, ref, sample)
        self.init_table(sc)
        self.zero_q_hits = 0  # light hits with cb >= 0 on a light with q == 0, over every path traced

    def connect(self, p, n, thr, st):
        if not self.use_table:
            return mr.MisRef.connect(self, p, n, thr, st)
        return self.connect_select(p, n, thr, st, True)

    def hit_weight(self, prim, t, o, d, cb):
        if not self.use_table:
            return mr.MisRef.hit_weight(self, prim, t, o, d, cb)
        ip = self.ip_of[int(prim)]
        if self.q_of[int(prim)] == 0:
            self.zero_q_hits += 1
            return F(1.0), False
        dd = fdot(d, d)
        d2 = (t * t) * dd
        inv = F(1.0) / np.sqrt(dd)
        om = tuple(d[i] * inv for i in range(3))
        nl = self.hits.normal(prim, t, o, d)[0]
        cos_l = np.abs(fdot(nl, om))
        A = self.area(prim)
        if cb > 0 and cos_l > 0 and d2 > 0 and A > 0:
            gh = (((cb * cos_l) * A) * ip) / (PI * d2)
            s = gh * gh
            if s < INF:
                return s / fmaf(gh, gh, F(1.0)), True
        return F(1.0), False


def render(ref, sc, w, h, frames, max_depth=pr.MAX_DEPTH, first=0, acc=None):
    """lit_scenes.render_nee's loop for frames first .. first + frames - 1 over any reference, going on from the
    accumulation `acc` ((h * w, 4), modified in place): (accumulation (h, w, 4), pixel words (h, w), segments,
    shadow rays among them)."""
    import emit_ref as er
    L = po.lib()
    acc = np.zeros((h * w, 4), F) if acc is None else acc
    px = np.zeros(h * w, np.uint32)
    total = shadow = 0
    for f in range(first, first + frames):
        rays, seeds = pr.camera_rays_seeds(sc, w, h, f)
        rad, nseg, _, _, _, nshadow = ref.paths_events(rays, seeds, max_depth)
        total += int(nseg.sum())
        shadow += int(nshadow.sum())
        rgb = np.ascontiguousarray(rad[:, :3])
        for i in range(h * w):
            px[i] = L.po_accumulate(acc[i].ctypes.data_as(er.PF), rgb[i].ctypes.data_as(er.PF), f)
    return acc.reshape(h, w, 4), px.reshape(h, w), total, shadow


@functools.lru_cache(maxsize=None)
def scene_refs(name):
    """(scene, SelectNeeRef, SelectMisRef, NeeRef, MisRef) of a scene of select_scenes.SCENES or lit_scenes.SETS,
    over one Ref."""
    import lit_scenes as ls
    import select_scenes as ss
    if name in ss.SCENES:
        from test_gpu_ray_query import Ref
        sc = ss.SCENES[name]()
        ref = Ref(sc)
    else:
        sc, nee, _ = ls.scene_refs(name)
        ref = nee.ref
    return sc, SelectNeeRef(sc, ref), SelectMisRef(sc, ref), nr.NeeRef(sc, ref), mr.MisRef(sc, ref)


def _frozen(out):
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case(name, mode, select=1, max_depth=pr.MAX_DEPTH):
    """(scene, rays, seeds, radiance, segments, ends, kinds, events, shadow rays) of a scene's ray set
    (select_scenes.rays_seeds) under light-sampling mode 1 or 2 with the selection on or off; computed once,
    never modified."""
    import select_scenes as ss
    refs = scene_refs(name)
    ref = refs[(1 if mode == 1 else 2) + (0 if select else 2)]
    rays, seeds = ss.rays_seeds(name)
    return (refs[0], rays, seeds) + _frozen(ref.paths_events(rays, seeds, max_depth))


@functools.lru_cache(maxsize=None)
def render_case(name, mode, w=32, h=24, frames=3, max_depth=pr.MAX_DEPTH):
    """(scene, accumulation (h, w, 4), pixel words (h, w), segments, shadow rays) of a render with the selection
    on; computed once, never modified."""
    refs = scene_refs(name)
    return (refs[0],) + _frozen(render(refs[1 if mode == 1 else 2], refs[0], w, h, frames, max_depth))
