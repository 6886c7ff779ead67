"""rt_denoise's rule (include/rt_hip.h) restated in vectorised numpy: every array and scalar has the
dtype of the context precision, every operation is one numpy ufunc call -- rounded once -- in the
order the header writes, and max / min are the header's comparisons (a > b ? a : b), so the device
can be held to these values bit for bit in fp32 and fp64."""
import numpy as np

DEFAULTS = dict(iterations=5, normal_log2_power=7, sigma_depth=0.05, sigma_lum=4.0, lum_eps=1e-6)
H5 = (0.0625, 0.25, 0.375, 0.25, 0.0625)   # the B3 spline, dx = -2 .. 2
G3 = (0.25, 0.5, 0.25)                     # the 3x3 Gaussian, dx = -1 .. 1


def e8(x):
    """u^8 by three squarings of u = max(1 - x / 8, 0), in x's dtype."""
    T = x.dtype.type
    u = T(1) - x * T(0.125)
    u = np.where(u > T(0), u, T(0))
    u = u * u
    u = u * u
    return u * u


def lum(c):
    return ((c[..., 0] + c[..., 1]) + c[..., 2]) / c.dtype.type(3)


def gather(img, dy, dx):
    """img[y + dy, x + dx] where that lies inside the image -> (values, inside); outside: the
    clamped cell's value, to be masked by `inside`."""
    Hh, Ww = img.shape[:2]
    ys, xs = np.arange(Hh)[:, None] + dy, np.arange(Ww)[None, :] + dx
    inside = (ys >= 0) & (ys < Hh) & (xs >= 0) & (xs < Ww)
    return img[np.clip(ys, 0, Hh - 1), np.clip(xs, 0, Ww - 1)], inside


def albedo_floor(T, H, W, albedo, hits, guide_samples):
    if albedo is None:
        return np.ones((H, W, 3), T)
    sky = (np.int64(guide_samples) - np.asarray(hits).reshape(H, W).astype(np.int64)).astype(T)
    v = (np.asarray(albedo, T).reshape(H, W, 3) + sky[..., None]) / T(guide_samples)
    return np.where(v > T(0.015625), v, T(0.015625))


def prepare(dtype, W, H, sums, sumsq, counts, samples, albedo, hits, normal, depth, guide_samples):
    """-> (c[H, W, 3], V[H, W], nhat[H, W, 3], z[H, W], a[H, W, 3])"""
    T = np.dtype(dtype).type
    s = np.asarray(sums, T).reshape(H, W, 3)
    n = (np.asarray(counts).reshape(H, W).astype(np.uint32) if counts is not None
         else np.full((H, W), samples, np.uint32))
    nT = n.astype(T)
    a = albedo_floor(T, H, W, albedo, hits, guide_samples)
    with np.errstate(all="ignore"):
        m = np.where(n[..., None] > 0, s / nT[..., None], T(0))
        c = m / a
        if sumsq is not None:
            q = np.asarray(sumsq, T).reshape(H, W, 3)
            d = q - s * m
            n1 = (n.astype(np.int64) - 1).astype(T)
            v = np.where(d > T(0), d / n1[..., None], T(0))
            v = v / (a * a)
            V = ((v[..., 0] + v[..., 1]) + v[..., 2]) / (T(3) * nT)
            V = np.where(n >= 2, V, T(0))
        else:
            L = lum(c)
            s1, s2, k = np.zeros((H, W), T), np.zeros((H, W), T), np.zeros((H, W), np.int64)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    Lq, inside = gather(L, dy, dx)
                    s1 = np.where(inside, s1 + Lq, s1)
                    s2 = np.where(inside, s2 + Lq * Lq, s2)
                    k += inside
            kT = k.astype(T)
            mu, mu2 = s1 / kT, s2 / kT
            d = mu2 - mu * mu
            V = np.where(d > T(0), d, T(0))
        nhat = np.zeros((H, W, 3), T)
        if normal is not None:
            N = np.asarray(normal, T).reshape(H, W, 3)
            d = (N[..., 0] * N[..., 0] + N[..., 1] * N[..., 1]) + N[..., 2] * N[..., 2]
            nhat = np.where((d > T(0))[..., None], N / np.sqrt(d)[..., None], T(0))
    z = np.asarray(depth, T).reshape(H, W) if depth is not None else np.zeros((H, W), T)
    return c.astype(T), V.astype(T), nhat.astype(T), z, a


def atrous_pass(c, V, nhat, z, step, normal_log2_power, sigma_depth, sigma_lum, lum_eps):
    """One pass of step `step` -> (c', V')."""
    T = c.dtype.type
    H, W = V.shape
    sd, sl, eps = T(sigma_depth), T(sigma_lum), T(lum_eps)
    with np.errstate(all="ignore"):
        vs, gs = np.zeros((H, W), T), np.zeros((H, W), T)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                Vq, inside = gather(V, dy, dx)
                g = T(G3[dx + 1]) * T(G3[dy + 1])
                vs = np.where(inside, vs + g * Vq, vs)
                gs = np.where(inside, gs + g, gs)
        den = sl * np.sqrt(vs / gs) + eps
        L = lum(c)
        flat = (nhat == T(0)).all(axis=-1)
        Sw, Sv, Sc = np.zeros((H, W), T), np.zeros((H, W), T), np.zeros((H, W, 3), T)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                k = T(H5[dx + 2]) * T(H5[dy + 2])
                cq, inside = gather(c, dy * step, dx * step)
                if dx == 0 and dy == 0:
                    w = np.full((H, W), k, T)
                else:
                    Vq, nq, zq, Lq, fq = (gather(i, dy * step, dx * step)[0] for i in (V, nhat, z, L, flat))
                    d = (nhat[..., 0] * nq[..., 0] + nhat[..., 1] * nq[..., 1]) + nhat[..., 2] * nq[..., 2]
                    t = np.where(d > T(0), d, T(0))
                    for _ in range(normal_log2_power):
                        t = t * t
                    wn = np.where(flat & fq, T(1), t)
                    differ = z != zq
                    dead = differ & (np.isinf(z) | np.isinf(zq))
                    xz = np.where(differ, np.abs(z - zq) / (sd * np.where(z < zq, z, zq)), T(0))
                    xl = np.abs(L - Lq) / den
                    w = np.where(dead, T(0), (k * wn) * e8(xz + xl))
                Vq = gather(V, dy * step, dx * step)[0]
                Sw = np.where(inside, Sw + w, Sw)
                Sc = np.where(inside[..., None], Sc + w[..., None] * cq, Sc)
                Sv = np.where(inside, Sv + (w * w) * Vq, Sv)
        return (Sc / Sw[..., None]).astype(T), (Sv / (Sw * Sw)).astype(T)


def denoise_ref(dtype, W, H, sums, sumsq=None, counts=None, samples=0, albedo=None, hits=None, normal=None,
                depth=None, guide_samples=0, **params):
    """rt_denoise -> (out[H W, 3], out_variance[H W]) in `dtype`.  params: DEFAULTS' fields."""
    p = dict(DEFAULTS, **params)
    c, V, nhat, z, a = prepare(dtype, W, H, sums, sumsq, counts, samples, albedo, hits, normal, depth, guide_samples)
    for i in range(p["iterations"]):
        c, V = atrous_pass(c, V, nhat, z, 1 << i, p["normal_log2_power"], p["sigma_depth"], p["sigma_lum"],
                           p["lum_eps"])
    return (c * a).reshape(H * W, 3), V.reshape(H * W)
