"""The reference of environment sampling (include/hippt.h HIPPT_OPT_ENV_SAMPLING): the map's selection
table in numpy integers and float32, and nee_ref.NeeRef / mis_ref.MisRef and their select_ref twins with the
connection, the coin and the miss replaced.  This file is the statement of record of the rule; the GPU matches the
table word for word and the paths bit for bit.

Every float operation below is one IEEE float32 operation in the association written; fdot, rand01, hash32 are the
oracle's, sg and env(d) env_ref's.  Everything reduced is a maximum or a sum of integers.

The table, over the map's texels E[y][x], S x S:

  uc = float(2x + 1) / float(S) - 1;  wc the same from y                       (the texel's centre)
  dy = (1 - |uc|) - |wc|;  (dx, dz) = (uc, wc) if dy >= 0 else ((1 - |wc|) * sg(uc), (1 - |uc|) * sg(wc))
  n2 = fdot(d, d);  J = 1 / (n2 * sqrt(n2))                (solid angle per unit of (u, w) area: 1 / |p|^3)
  lum = (E.r + E.g) + E.b;  W = lum * J;  W = W if W > 0 and W < +inf else 0
  per row y:  Wmax_y = max_x W;  q(x,y) = min(4096, max(1, int((W / Wmax_y) * 4096))) if Wmax_y > 0 else 1
              c(x,y) = q(0,y) + ... + q(x,y);  R_y = c(S-1, y);  V_y = (float(R_y) * 2^-12) * Wmax_y
  over rows:  Vmax = max_y V_y;  flat = not (Vmax > 0 and Vmax < +inf)
              m_y = 1 if flat else min(65536, max(1, int((V_y / Vmax) * 65536)));  C_y = m_0 + ... + m_y;  T = C_{S-1}
  per texel:  k(x,y) = ((float(m_y) / float(T)) * (float(q) / float(R_y))) * (0.25 * (float(S) * float(S)))

The connection, at a Lambertian vertex after po_scatter (thr', faced normal n; nL emissive primitives):

  sel = 1
  if nL > 0:  c0 = rand01;  sel = 0.5;  if not c0 < 0.5: the light connection of the mode and of the light selection
              with (nl * 2) where nl (float(nLights) or ip_k) stands; done
  rng = hash32(rng);  xr = (rng * T) >> 32 in 64 bits;    y = the smallest row with C_y > xr
  rng = hash32(rng);  xc = (rng * R_y) >> 32;             x = the smallest column with c(x,y) > xc
  a = rand01;  b = rand01;  g2 = 2 / float(S);  u = fmaf(float(x) + a, g2, -1);  w = fmaf(float(y) + b, g2, -1)
  d from (u, w) as above;  n2 = fdot(d, d);  om = d * (1 / sqrt(n2));  cosS = fdot(n, om)
  pl = (k(x,y) * (n2 * sqrt(n2))) * sel;  no shadow ray unless cosS > 0 and pl > 0 (the draws are consumed)
  g = cosS / (3.14159274 * pl)
  mode 1: Ld = (thr' * env(om)) * g;   mode 2: no shadow ray unless g < +inf; Ld = (thr' * env(om)) * (g / fmaf(g, g, 1))
  the shadow ray (p, om), tmin 0.001, no tmax: Lacc += Ld iff it has no hit at all; a segment and a shadow ray.

The * 2 also enters the MIS weight of a light hit.  A segment of direction d that misses:

  no Lambertian scatter before it:       L = Lacc + thr * env(d)
  mode 1, after a Lambertian scatter:    L = Lacc
  mode 2, after a Lambertian scatter:    L = Lacc + (thr * env(d)) * wb, wb = 1 unless
      s1 = (|dx| + |dy|) + |dz|;  r = sqrt(fdot(d, d)) / s1;  r3 = (r * r) * r;  (u, w) = env_ref.coords(d);  h = 0.5 * S
      x = int(fmin(fmax(fmaf(u, h, h), 0), S - 1));  y the same from w;  pl = (k(x,y) * r3) * sel
      cb > 0 and pl > 0:  gh = cb / (3.14159274 * pl);  s = gh * gh;  s < +inf:  wb = s / fmaf(gh, gh, 1)

k >= 2^-28 * 2^-24 * 0.25 and |p|^3 >= 3^-1.5, so pl >= 2^-57: g and gh stay below 2^59 and "g is not below +inf"
cannot happen; the condition stands in the rule (and in the kernel) for symmetry with the lights', and INFINITE_G_ENV
is never set (tests/test_envs_ref_cpu.py asserts it)."""
import ctypes
import functools

import numpy as np

import env_ref
import hippt
import mis_ref as mr
import nee_ref as nr
import path_ref as pr
import pyoracle as po
import select_ref as sr
from hippt import scenes
from hit_ref import f3, fdot, fmaf
from nee_ref import ABSORBED, DEPTH, EMITTED, INVALID, MISS, PI, F, INF  # noqa: F401

Q_ONE = 4096
M_ONE = 65536
ROW_DTYPE = hippt.ENV_ROW_DTYPE
TEXEL_DTYPE = hippt.ENV_TEXEL_DTYPE

# further event bits (detail["events"]) beside nee_ref's, mis_ref's and select_ref's
ENV_VISIBLE = 1 << 12        # a shadow ray to the map had no hit, with Ld > 0
ENV_OCCLUDED = 1 << 13       # a shadow ray to the map hit something
ENV_BACKFACING = 1 << 14     # no shadow ray: cosS <= 0 for the drawn direction
INFINITE_G_ENV = 1 << 15     # no shadow ray: g is not below +inf (cannot happen: the module's last paragraph)
COIN_LIGHTS = 1 << 16        # the coin sent a vertex to the lights
COIN_MAP = 1 << 17           # the coin sent a vertex to the map
WEIGHTED_MISS = 1 << 18      # mode 2: a miss after a Lambertian scatter whose wb came from the formula
UNWEIGHTED_MISS_AFTER_DIFFUSE = 1 << 19  # a miss after a Lambertian scatter taken whole (mode 2, wb = 1) or not at all (mode 1)
FLOOR_TEXEL = 1 << 20        # the drawn texel's q is the floor, 1, in a row that is not flat
LOWER_DRAWN = 1 << 21        # the drawn direction points below the horizon
EVENTS = dict(sr.EVENTS, **{"env visible": ENV_VISIBLE, "env occluded": ENV_OCCLUDED, "env backfacing": ENV_BACKFACING,
                            "env infinite g": INFINITE_G_ENV, "coin lights": COIN_LIGHTS, "coin map": COIN_MAP,
                            "weighted miss": WEIGHTED_MISS, "unweighted miss after diffuse": UNWEIGHTED_MISS_AFTER_DIFFUSE,
                            "floor texel": FLOOR_TEXEL, "lower drawn": LOWER_DRAWN})


def vfmaf(a, b, c):
    """fmaf over float32 arrays, correctly rounded: the product is exact in float64, the sum is rounded to odd there
    (truncated, the sticky bit set), and 53 >= 2 * 24 + 2 bits make the final rounding to float32 the exact one."""
    a, b, c = (np.asarray(v, np.float64) for v in np.broadcast_arrays(a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        inexact = (err != 0) & np.isfinite(s)
        shrink = inexact & ((err > 0) != (s > 0))  # the exact sum is smaller in magnitude than s
        t = np.where(shrink, np.nextafter(s, 0.0), s)
        bits = np.ascontiguousarray(t).view(np.int64) | inexact.astype(np.int64)
        return bits.view(np.float64).astype(F)


def oct_point(u, w):
    """The octahedron's point above (u, w), scalars: (dx, dy, dz) float32."""
    u, w = F(u), F(w)
    dy = (F(1.0) - np.abs(u)) - np.abs(w)
    if dy >= 0:
        return u, dy, w
    return (F(1.0) - np.abs(w)) * env_ref.sg(u), dy, (F(1.0) - np.abs(u)) * env_ref.sg(w)


def weights(E):
    """W (S, S) float32 of the map E (S, S, 3)."""
    E = np.asarray(E, F)
    size = E.shape[0]
    with np.errstate(all="ignore"):
        c = (2 * np.arange(size, dtype=np.int64) + 1).astype(F) / F(size) - F(1.0)
        uc, wc = np.broadcast_arrays(c[None, :], c[:, None])
        au, aw = np.abs(uc), np.abs(wc)
        dy = (F(1.0) - au) - aw
        up = dy >= 0
        dx = np.where(up, uc, (F(1.0) - aw) * np.where(uc < 0, F(-1.0), F(1.0))).astype(F)
        dz = np.where(up, wc, (F(1.0) - au) * np.where(wc < 0, F(-1.0), F(1.0))).astype(F)
        n2 = vfmaf(dx, dx, vfmaf(dy, dy, dz * dz))
        J = F(1.0) / (n2 * np.sqrt(n2))
        lum = (E[..., 0] + E[..., 1]) + E[..., 2]
        W = (lum * J).astype(F)
        return np.where((W > 0) & (W < INF), W, F(0.0)).astype(F)


def table(E):
    """The selection table of the map E (S, S, 3) float32: {"rows": structured (S,) with m, C; "texels": structured
    (S, S) with q, c, k}."""
    E = np.asarray(E, F)
    size = E.shape[0]
    assert E.shape == (size, size, 3)
    W = weights(E)
    with np.errstate(all="ignore"):
        wmax = W.max(axis=1)
        lit = wmax > 0
        ratio = ((W / np.where(lit, wmax, F(1.0))[:, None]) * F(Q_ONE)).astype(F)
        q = np.where(lit[:, None], np.minimum(Q_ONE, np.maximum(1, ratio.astype(np.int64))), 1).astype(np.uint32)
        c = np.cumsum(q.astype(np.uint64), axis=1)
        R = c[:, -1]
        assert int(R.max()) <= 1 << 24
        V = ((R.astype(F) * F(0.000244140625)) * wmax).astype(F)
        vmax = F(V.max())
        flat = not (vmax > 0 and vmax < INF)
        if flat:
            m = np.ones(size, np.uint32)
        else:
            m = np.minimum(M_ONE, np.maximum(1, ((V / vmax) * F(M_ONE)).astype(F).astype(np.int64))).astype(np.uint32)
        C = np.cumsum(m.astype(np.uint64))
        T = int(C[-1])
        assert size <= T <= 1 << 28
        k = (((m.astype(F) / F(T))[:, None] * (q.astype(F) / R.astype(F)[:, None])) *
             (F(0.25) * (F(size) * F(size)))).astype(F)
    rows = np.zeros(size, ROW_DTYPE)
    rows["m"], rows["C"] = m, C.astype(np.uint32)
    tex = np.zeros((size, size), TEXEL_DTYPE)
    tex["q"], tex["c"], tex["k"] = q, c.astype(np.uint32), k
    return {"rows": rows, "texels": tex}


def selection_probability(tab, x, y):
    """(numerator, denominator) of texel (x, y)'s selection probability m_y q / (T R_y), exact integers."""
    rows, tex = tab["rows"], tab["texels"]
    return int(rows["m"][y]) * int(tex["q"][y, x]), int(rows["C"][-1]) * int(tex["c"][y, -1])


def draw(tab, st):
    """One draw from the table with RNG state st (a ctypes.c_uint32, advanced by four draws): dict of x, y, om (the
    unit direction), n3 = n2 * sqrt(n2), k, and d (the unnormalised direction)."""
    L = po.lib()
    rows, tex = tab["rows"], tab["texels"]
    size = len(rows)
    L.po_rand01(ctypes.byref(st))
    xr = (int(st.value) * int(rows["C"][-1])) >> 32
    y = int(np.searchsorted(rows["C"], xr, side="right"))
    L.po_rand01(ctypes.byref(st))
    xc = (int(st.value) * int(tex["c"][y, -1])) >> 32
    x = int(np.searchsorted(tex["c"][y], xc, side="right"))
    a = F(L.po_rand01(ctypes.byref(st)))
    b = F(L.po_rand01(ctypes.byref(st)))
    g2 = F(2.0) / F(size)
    u = fmaf(F(x) + a, g2, F(-1.0))
    w = fmaf(F(y) + b, g2, F(-1.0))
    d = oct_point(u, w)
    n2 = fdot(d, d)
    inv = F(1.0) / np.sqrt(n2)
    return {"x": x, "y": y, "om": tuple(d[i] * inv for i in range(3)), "n3": n2 * np.sqrt(n2), "k": F(tex["k"][y, x]),
            "d": d}


def connect_factor(k, n3, cos_s, sel, mis):
    """(g or the MIS factor, why no shadow ray is traced: 0, ENV_BACKFACING or INFINITE_G_ENV; None factor then)."""
    with np.errstate(all="ignore"):
        pl = (F(k) * F(n3)) * F(sel)
        if not cos_s > 0:
            return None, ENV_BACKFACING
        if not pl > 0:
            return None, 0
        g = F(cos_s) / (PI * pl)
        if mis:
            if not g < INF:
                return None, INFINITE_G_ENV
            g = g / fmaf(g, g, F(1.0))
    return g, 0


def miss_weight(tab, d, cb, sel):
    """(wb of a miss of direction d after a Lambertian scatter of cosine cb, whether the formula gave it)."""
    size = len(tab["rows"])
    d = f3(d)
    with np.errstate(all="ignore"):
        s1 = (np.abs(d[0]) + np.abs(d[1])) + np.abs(d[2])
        r = np.sqrt(fdot(d, d)) / s1
        r3 = (r * r) * r
        u, w = env_ref.coords(d)
        h = F(0.5) * F(size)
        x = int(np.fmin(np.fmax(fmaf(u, h, h), F(0.0)), F(size - 1)))
        y = int(np.fmin(np.fmax(fmaf(w, h, h), F(0.0)), F(size - 1)))
        pl = (F(tab["texels"]["k"][y, x]) * r3) * F(sel)
        if cb > 0 and pl > 0:
            gh = F(cb) / (PI * pl)
            s = gh * gh
            if s < INF:
                return s / fmaf(gh, gh, F(1.0)), True
    return F(1.0), False


class _EnvSampling:
    """What the four references share: the map, its table, the coin, the connection to the map, the light connection
    and the light hit's weight with the coin's factor, and the path."""

    mis = False
    select = False

    def init_env(self, E):
        self.E = np.ascontiguousarray(E, F)
        self.etab = table(self.E)
        self.size = self.E.shape[0]
        self.sel = F(0.5) if self.lights else F(1.0)
        q = self.etab["texels"]["q"]
        self.row_has_floor = q.max(axis=1) > 1
        self.use_light_table = self.select and 0 < len(self.lights) <= sr.LIGHT_MAX

    # ---- the lights, with the coin's factor 2 ----
    def light_connect2(self, p, n, thr, st):
        """NeeRef's / MisRef's / select_ref's connection with (nl * 2) where nl stands."""
        nl_count = len(self.lights)
        note = 0
        if self.use_light_table:
            k, ip = self.pick(st)
            if k is None:
                return None, (F(0.0), F(0.0), F(0.0)), -2, sr.NO_LIGHT
            if self.floor_matters and self.q_of[k] == 1:
                note = sr.FLOOR_SELECTED
        else:
            u0 = F(po.lib().po_rand01(ctypes.byref(st)))
            k = self.lights[min(int(u0 * F(nl_count)), nl_count - 1)]
            ip = F(nl_count)
        om, cos_s, cos_l, d2, A, why = sr._Select.geometry(self, k, p, n, st)
        with np.errstate(all="ignore"):
            if not cos_s > 0 or not cos_l > 0 or not d2 > 0 or not A > 0:
                return None, om, k, why | note
            g = (((cos_s * cos_l) * A) * (ip * F(2.0))) / (PI * d2)
            if self.mis:
                if not g < INF:
                    return None, om, k, mr.INFINITE_G | note
                g = g / fmaf(g, g, F(1.0))
            le = self.prim_emission[k]
            return tuple((F(thr[i]) * le[i]) * g for i in range(3)), om, k, note

    def hit_weight2(self, prim, t, o, d, cb):
        """MisRef's / SelectMisRef's wb of a light hit with (nl * 2) where nl stands."""
        if self.use_light_table:
            if self.q_of[int(prim)] == 0:
                return F(1.0), False
            nl = self.ip_of[int(prim)]
        else:
            nl = F(len(self.lights))
        with np.errstate(all="ignore"):
            dd = fdot(d, d)
            d2 = (t * t) * dd
            inv = F(1.0) / np.sqrt(dd)
            om = tuple(d[i] * inv for i in range(3))
            cos_l = np.abs(fdot(self.hits.normal(prim, t, o, d)[0], om))
            A = mr.MisRef.area(self, prim)
            if cb > 0 and cos_l > 0 and d2 > 0 and A > 0:
                gh = (((cb * cos_l) * A) * (nl * F(2.0))) / (PI * d2)
                s = gh * gh
                if s < INF:
                    return s / fmaf(gh, gh, F(1.0)), True
        return F(1.0), False

    # ---- the map ----
    def env_connect(self, n, thr, st):
        """(Ld or None, om, -1, events)."""
        dr = draw(self.etab, st)
        note = COIN_MAP if self.lights else 0
        if dr["om"][1] < 0:
            note |= LOWER_DRAWN
        if self.row_has_floor[dr["y"]] and int(self.etab["texels"]["q"][dr["y"], dr["x"]]) == 1:
            note |= FLOOR_TEXEL
        cos_s = fdot(n, dr["om"])
        g, why = connect_factor(dr["k"], dr["n3"], cos_s, self.sel, self.mis)
        if g is None:
            return None, dr["om"], -1, note | why
        e = env_ref.lookup(self.E, dr["om"])
        with np.errstate(all="ignore"):
            return tuple((F(thr[i]) * e[i]) * g for i in range(3)), dr["om"], -1, note

    def connect(self, p, n, thr, st):
        """The vertex's one connection: (Ld or None, om, light id or -1 for the map, events)."""
        if self.lights:
            c0 = F(po.lib().po_rand01(ctypes.byref(st)))
            if not c0 < F(0.5):
                ld, om, k, why = self.light_connect2(p, n, thr, st)
                return ld, om, k, why | COIN_LIGHTS
        return self.env_connect(n, thr, st)

    def path(self, ray, seed, max_depth, detail=None):
        """(rgba (4,) float32, segments, how it ended, bit mask of the material kinds it scattered at); detail as
        NeeRef.path's."""
        out = np.zeros(4, F)
        if detail is not None:
            detail["events"], detail["shadow"] = 0, 0
        if not pr.valid(ray):
            return out, 0, INVALID, 0
        o = (ctypes.c_float * 3)(*[float(x) for x in ray[0:3]])
        d = (ctypes.c_float * 3)(*[float(x) for x in ray[4:7]])
        thr = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
        st = ctypes.c_uint32(int(seed) & 0xFFFFFFFF)
        seg = np.zeros((1, 8), F)
        lacc = np.zeros(3, F)
        diffuse = False  # the last scatter was Lambertian (mode 1: not spec; mode 2: not cb < 0)
        cb = F(-1.0)
        segs, kinds, end, events, shadow = 0, 0, DEPTH, 0, 0
        with np.errstate(all="ignore"):
            for depth in range(max_depth):
                seg[0, 0:3], seg[0, 4:7] = o[:], d[:]
                seg[0, 3], seg[0, 7] = (ray[3], ray[7]) if depth == 0 else (F(0.001), INF)
                t, p = self.ref.closest(seg)
                segs += 1
                prim = int(p[0])
                if prim < 0:
                    e = env_ref.lookup(self.E, f3(d))
                    base = np.array([F(thr[i]) * e[i] for i in range(3)], F)
                    if not diffuse:
                        out[0:3] = lacc + base
                    elif not self.mis:
                        out[0:3] = lacc
                        events |= UNWEIGHTED_MISS_AFTER_DIFFUSE
                    else:
                        wb, formula = miss_weight(self.etab, f3(d), cb, self.sel)
                        out[0:3] = lacc + base * wb
                        events |= WEIGHTED_MISS if formula else UNWEIGHTED_MISS_AFTER_DIFFUSE
                    end = MISS
                    break
                if depth == 0:
                    out[3] = 1.0
                if self.prim_kind[prim] == scenes.MAT_EMISSIVE:  # before the depth check
                    le = np.array(thr[:], F) * self.prim_emission[prim]
                    if not diffuse:
                        out[0:3] = lacc + le
                        events |= nr.LIGHT_SPECULAR
                    elif not self.mis:
                        out[0:3] = lacc
                        events |= nr.LIGHT_AFTER_DIFFUSE
                    else:
                        wb, formula = self.hit_weight2(prim, F(t[0]), f3(o), f3(d), cb)
                        out[0:3] = lacc + le * wb
                        events |= nr.LIGHT_AFTER_DIFFUSE | (mr.WEIGHTED_HIT if formula else mr.UNWEIGHTED_HIT_AFTER_DIFFUSE)
                    end = EMITTED
                    break
                if depth + 1 >= max_depth:
                    out[0:3] = lacc
                    break
                kind = int(self.prim_kind[prim])
                kinds |= 1 << kind
                n = self.hits.normal(prim, F(t[0]), f3(o), f3(d))[1]
                if not self.L.po_scatter(self.ora.handle, prim, float(t[0]), o, d, ctypes.byref(st), thr):
                    out[0:3] = lacc
                    end = ABSORBED
                    break
                diffuse = kind == scenes.MAT_LAMBERTIAN
                if not diffuse:
                    cb = F(-1.0)
                    continue
                sd = f3(d)
                cb = fdot(n, sd) * (F(1.0) / np.sqrt(fdot(sd, sd)))
                if self.mis and cb < 0:  # (the rule's test is cb < 0: a negative cosine reads as "not Lambertian")
                    diffuse = False
                ld, om, k, why = self.connect(f3(o), n, thr, st)
                events |= why
                if ld is None:
                    continue
                seg[0, 0:3], seg[0, 4:7] = o[:], om
                seg[0, 3], seg[0, 7] = F(0.001), INF
                _, sp = self.ref.closest(seg)
                segs += 1
                shadow += 1
                if self.mis:
                    events |= mr.WEIGHTED_CONNECTION
                hit = int(sp[0])
                if k == -1:
                    if hit < 0:
                        lacc = lacc + np.array(ld, F)
                        if max(ld) > 0:
                            events |= ENV_VISIBLE
                    else:
                        events |= ENV_OCCLUDED
                elif hit == k:
                    lacc = lacc + np.array(ld, F)
                    if max(ld) > 0:
                        events |= nr.VISIBLE
                else:
                    events |= nr.OCCLUDED
            else:
                out[0:3] = lacc
        if detail is not None:
            detail["events"], detail["shadow"] = events, shadow
        return out, segs, end, kinds


class EnvNeeRef(_EnvSampling, nr.NeeRef):
    """nee_ref.NeeRef under the map E with HIPPT_OPT_ENV_SAMPLING."""

    def __init__(self, sc, ref, E):
        nr.NeeRef.__init__(self, sc, ref)
        self.init_env(E)


class EnvMisRef(_EnvSampling, mr.MisRef):
    """mis_ref.MisRef under the map E with HIPPT_OPT_ENV_SAMPLING."""
    mis = True

    def __init__(self, sc, ref, E):
        mr.MisRef.__init__(self, sc, ref)
        self.init_env(E)


class EnvSelectNeeRef(_EnvSampling, sr.SelectNeeRef):
    """select_ref.SelectNeeRef under the map E with HIPPT_OPT_ENV_SAMPLING."""
    select = True

    def __init__(self, sc, ref, E):
        sr.SelectNeeRef.__init__(self, sc, ref)
        self.init_env(E)


class EnvSelectMisRef(_EnvSampling, sr.SelectMisRef):
    """select_ref.SelectMisRef under the map E with HIPPT_OPT_ENV_SAMPLING."""
    mis = True
    select = True

    def __init__(self, sc, ref, E):
        sr.SelectMisRef.__init__(self, sc, ref)
        self.init_env(E)


def ref_class(mode, select=False):
    return {(1, False): EnvNeeRef, (2, False): EnvMisRef, (1, True): EnvSelectNeeRef, (2, True): EnvSelectMisRef}[
        (int(mode), bool(select))]


def _frozen(out):
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return tuple(out)


# ---- maps and scenes of the tests ------------------------------------------------------------------------------
def sun_block(size, y0, x0, ratio=1.0e4, base=0.05, n=2):
    """A map (S, S, 3) of `base` with an n x n block at (y0, x0) `ratio` times that."""
    E = np.full((size, size, 3), base, F)
    E[y0:y0 + n, x0:x0 + n] = F(base * ratio)
    return np.ascontiguousarray(E)


@functools.lru_cache(maxsize=None)
def test_env(size, kind="random"):
    """The maps of the path tests: "random" is env_ref.random_env (five decades and zero texels, so every row has
    floor texels); "block" a dim map with a 2 x 2 block 10^4 times the rest in the upper hemisphere."""
    if kind == "block":
        return _frozen([sun_block(size, size // 2, size // 2 + size // 8, n=2 if size >= 8 else 1)])[0]
    return _frozen([np.array(env_ref.random_env(size, 3))])[0]


def open_box():
    """A small closed scene opening to the map: a Lambertian floor, three walls and a ceiling with a square hole,
    seen from the open fourth side; no light.  28 triangles."""
    v, mats = [], []

    def quad(a, b, c, d, m):
        v.append([*a, *b, *c])
        v.append([*a, *c, *d])
        mats.extend([m, m])

    lo, hi = -1.0, 1.0
    quad((lo, 0, lo), (hi, 0, lo), (hi, 0, hi), (lo, 0, hi), 0)            # floor
    quad((lo, 0, lo), (lo, 2, lo), (hi, 2, lo), (hi, 0, lo), 1)            # back wall
    quad((lo, 0, lo), (lo, 0, hi), (lo, 2, hi), (lo, 2, lo), 2)            # left wall
    quad((hi, 0, lo), (hi, 2, lo), (hi, 2, hi), (hi, 0, hi), 1)            # right wall
    h = 0.4  # the ceiling, y = 2, with the hole [-h, h]^2
    quad((lo, 2, lo), (lo, 2, -h), (hi, 2, -h), (hi, 2, lo), 0)
    quad((lo, 2, h), (lo, 2, hi), (hi, 2, hi), (hi, 2, h), 0)
    quad((lo, 2, -h), (lo, 2, h), (-h, 2, h), (-h, 2, -h), 0)
    quad((h, 2, -h), (h, 2, h), (hi, 2, h), (hi, 2, -h), 0)
    quad((-0.4, 0, -0.4), (-0.4, 0.6, -0.4), (0.3, 0.6, -0.4), (0.3, 0, -0.4), 2)   # a blocker on the floor
    quad((-0.4, 0.6, -0.4), (-0.4, 0.6, 0.3), (0.3, 0.6, 0.3), (0.3, 0.6, -0.4), 2)
    albedo = np.array([[0.73, 0.73, 0.73], [0.65, 0.25, 0.2], [0.2, 0.45, 0.3]], np.float32)
    return scenes.Scene("open_box", np.array(v, np.float32), np.array(mats, np.int32), albedo,
                        lookfrom=(0.0, 1.0, 3.4), lookat=(0.0, 0.9, 0.0), vfov=40.0)


@functools.lru_cache(maxsize=None)
def scene_of(name):
    """(scene, its test_gpu_ray_query.Ref) of "open_box", a lit scene of emit_ref.LIT / select_scenes.SCENES /
    lit_scenes.SETS, or a scene of test_gpu_ray_query.case."""
    import emit_ref as er
    import lit_scenes as ls
    import select_scenes as ss
    from test_gpu_ray_query import Ref, case
    if name == "open_box":
        sc = open_box()
        return sc, Ref(sc)
    if name in ss.SCENES:
        refs = sr.scene_refs(name)
        return refs[0], refs[3].ref
    if name in ls.SETS:
        sc, nee, _ = ls.scene_refs(name)
        return sc, nee.ref
    if name in er.LIT:
        sc, nee = nr.scene_ref(name)
        return sc, nee.ref
    sc = case(name)[0]
    return sc, Ref(sc)


@functools.lru_cache(maxsize=None)
def rays_of(name, n=1025):
    """(rays, seeds) of a scene's ray set: test_gpu_ray_query.make_rays(sc, n), path_seeds(n, 0); never modified."""
    from test_gpu_ray_query import make_rays
    sc, _ = scene_of(name)
    rays = make_rays(sc, n)
    seeds = hippt.path_seeds(len(rays), pr.SEED_FRAME)
    return _frozen([rays, seeds])


# The ray sets of tests/test_gpu_env_sampling.py: (scene, map size, map kind, light selection by power).  The four
# scenes without a light of tests/test_gpu_environment.py, the open box under the block map, other sizes, and lit
# scenes (the coin) with both light selections.
PATH_CASES = (("cornell34", 5, "random", False), ("cornell_mixed", 5, "random", False), ("blob64x34", 5, "random", False),
              ("random_scene", 5, "random", False), ("open_box", 64, "block", False), ("cornell34", 1, "random", False),
              ("cornell_mixed", 64, "random", False), ("cornell34_lit", 5, "random", False),
              ("cornell_mixed_lit", 64, "random", False), ("cornell34_lit", 5, "random", True))


def case_id(c):
    return f"{c[0]}-S{c[1]}-{c[2]}" + ("-select" if c[3] else "")


@functools.lru_cache(maxsize=None)
def case(name, mode, size, kind="random", select=False, max_depth=pr.MAX_DEPTH, n=1025):
    """(scene, map, rays, seeds, radiance, segments, ends, kinds, events, shadow rays) of a scene's ray set under the
    map test_env(size, kind) with environment sampling; computed once, never modified."""
    sc, ref = scene_of(name)
    E = test_env(size, kind)
    rays, seeds = rays_of(name, n)
    r = ref_class(mode, select)(sc, ref, E)
    return (sc, E, rays, seeds) + _frozen(r.paths_events(rays, seeds, max_depth))


@functools.lru_cache(maxsize=None)
def render_case(name, mode, size, kind="random", select=False, w=32, h=24, frames=3, max_depth=pr.MAX_DEPTH):
    """(scene, map, accumulation (h, w, 4), pixel words (h, w), segments, shadow rays) of a render with environment
    sampling; computed once, never modified."""
    sc, ref = scene_of(name)
    E = test_env(size, kind)
    r = ref_class(mode, select)(sc, ref, E)
    return (sc, E) + _frozen(sr.render(r, sc, w, h, frames, max_depth))
