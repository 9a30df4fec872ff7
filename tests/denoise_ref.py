"""The numpy float32 model of the denoiser's contract (include/hippt.h hipptDenoise),
written from the contract's text: every sum, product and quotient below is one float32 operation on
float32 operands, in the order the contract writes it; no fused multiply-add, no exp or pow.

Per pixel p, with c(p) the accumulation's rgb and the hit record of the guide sample (t, prim, normal,
matFlags):
  albedo'(p)  per channel the material's albedo where p is a hit, its material is Lambertian and the
              channel is >= 2^-6, else 1;  i_0(p) = c(p) / albedo'(p)
  pass k      s = 2^k, sigma = sigmaColor * (1 / float(s)), zden(p) = sigmaDepth * (t_p * float(s));
              a sky pixel keeps i_k(p); a hit pixel sums over the taps q = (x + dx s, y + dy s), dy = -2..2
              outside and dx = -2..2 inside, skipping q outside the image or over the sky:
                h = K[|dy|] K[|dx|], K = {3/8, 1/4, 1/16}
                dn = max(0, (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z), wn = dn squared normalPower times
                xz = |t_p - t_q| / zden(p), wz = 1 / (1 + xz xz)
                d = i_k(p) - i_k(q), dc = (d.x d.x + d.y d.y) + d.z d.z, wc = 1 / (1 + dc / sigma^2)
                w = ((h wn) wz) wc;  sum.ch = sum.ch + w i_k(q).ch;  wsum = wsum + w   (from +0)
              i_{k+1}(p) = sum / wsum
  output      rgba(p) = (i_passes(p) * albedo'(p), 1); the word is pack_pixel of it.

guides() builds the hit records of a camera sample from the oracle-pinned references of the ray-query
tests (test_gpu_ray_query.Ref / camera_rays, hit_ref.HitRef)."""
import numpy as np

F = np.float32
MATERIAL_MASK = (1 << 30) - 1
MAT_LAMBERTIAN = 0
MIN_ALBEDO = F(2.0 ** -6)
K = (F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0))
PIXEL_ARGB, PIXEL_RGBA8 = 0, 1


def guides(sc, w, h, frame=0):
    """The hit records (HIT_DTYPE, (h, w)) of sample `frame`'s camera rays over scene sc."""
    from hit_ref import HitRef
    from test_gpu_ray_query import Ref, camera_rays
    ref = Ref(sc)
    rays = camera_rays(sc, w, h, frame)
    t, prim = ref.closest(rays)
    return HitRef(sc, ref).records(rays, t, prim).reshape(h, w)


def albedo_prime(hits, materials, demodulate=True):
    """albedo' (H, W, 3) float32."""
    hit = hits["prim"] >= 0
    out = np.ones(hit.shape + (3,), F)
    if not demodulate:
        return out
    idx = np.where(hit, hits["matFlags"] & MATERIAL_MASK, 0)
    lamb = hit & (np.asarray(materials["kind"])[idx] == MAT_LAMBERTIAN)
    alb = np.asarray(materials["albedo"], F).reshape(-1, 3)[idx]
    use = lamb[..., None] & (alb >= MIN_ALBEDO)
    out[use] = alb[use]
    return out


def one_pass(i, hits, k, sigma_color, sigma_depth, normal_power):
    h_, w_ = hits.shape
    s = 1 << k
    fs = F(s)
    sigma = F(sigma_color) * (F(1.0) / fs)
    sigma2 = F(sigma * sigma)
    t = hits["t"].astype(F)
    n = hits["normal"].astype(F)
    hit = hits["prim"] >= 0
    zden = F(sigma_depth) * (t * fs)
    ys, xs = np.mgrid[0:h_, 0:w_]
    total = np.zeros((h_, w_, 3), F)
    wsum = np.zeros((h_, w_), F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            yq, xq = ys + dy * s, xs + dx * s
            inside = (yq >= 0) & (yq < h_) & (xq >= 0) & (xq < w_)
            yc, xc = np.clip(yq, 0, h_ - 1), np.clip(xq, 0, w_ - 1)
            take = inside & hit[yc, xc]
            iq, nq, tq = i[yc, xc], n[yc, xc], t[yc, xc]
            hk = F(K[abs(dy)] * K[abs(dx)])
            dn = np.fmax(F(0.0), (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
            wn = dn
            for _ in range(normal_power):
                wn = wn * wn
            xz = np.abs(t - tq) / zden
            wz = F(1.0) / (F(1.0) + xz * xz)
            d = i - iq
            dc = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            wc = F(1.0) / (F(1.0) + dc / sigma2)
            wgt = ((hk * wn) * wz) * wc
            assert wgt.dtype == F and iq.dtype == F
            total = np.where(take[..., None], total + wgt[..., None] * iq, total)
            wsum = np.where(take, wsum + wgt, wsum)
    out = total / wsum[..., None]
    return np.where(hit[..., None], out, i).astype(F)


def filtered(accum, hits, materials, passes=5, sigma_color=1.0, sigma_depth=0.05, normal_power=6, demodulate=True):
    """rgba (H, W, 4) float32 of the contract, from the accumulation (H, W, 4) and the guide records."""
    c = np.ascontiguousarray(accum, F)[..., :3]
    ap = albedo_prime(hits, materials, demodulate)
    with np.errstate(all="ignore"):
        i = c / ap
        assert i.dtype == F
        for k in range(passes):
            i = one_pass(i, hits, k, sigma_color, sigma_depth, normal_power)
        out = np.ones(i.shape[:2] + (4,), F)
        out[..., :3] = i * ap
    return out


def pack_pixel(rgb, fmt=PIXEL_ARGB):
    """The renderer's pixel word (include/hippt.h "Output frame word formats") of linear colours (..., >= 3)."""
    c = np.asarray(rgb, F)[..., :3]
    with np.errstate(all="ignore"):
        x = np.sqrt(np.fmin(np.fmax(c, F(0.0)), F(1.0))) * F(255.0)
    assert x.dtype == F
    if fmt == PIXEL_RGBA8:
        q = np.rint(x).astype(np.uint32)
        return (np.uint32(255) << 24) | (q[..., 2] << 16) | (q[..., 1] << 8) | q[..., 0]
    q = x.astype(np.uint32)  # truncated
    return (np.uint32(255) << 24) | (q[..., 0] << 16) | (q[..., 1] << 8) | q[..., 2]


def denoise(accum, hits, materials, fmt=PIXEL_ARGB, **kw):
    """(pixels (H, W) uint32, rgba (H, W, 4) float32): what PathTracer.denoise returns."""
    rgba = filtered(accum, hits, materials, **kw)
    return pack_pixel(rgba, fmt).astype(np.uint32), rgba
