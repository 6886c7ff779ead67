"""The rules of rt_render_pixels_moments and rt_refine_jobs (include/rt_hip.h), restated for the
CPU: f32_sumsq / f64_sumsq (the per-job second moment from per-sample radiance) and refine_ref
(one adaptive round over a job list, in numpy float64)."""
import numpy as np

from raytracingproject_amd import _native as N


def f32_sumsq(L: np.ndarray, counts, start=None) -> np.ndarray:
    """L[T, 3] float32 per-sample radiance, job k owning the next counts[k] rows -> float32[len(counts),
    3].  Per channel r = rintf(L 2^19); r == 0 adds nothing, a NaN r makes the channel NaN, |r| >=
    2^32 makes it +inf (NaN wins); otherwise r r, an exact integer, joins two words: S_lo += r r &
    0xffffffff, S_hi += r r >> 32.  out = (float)(((double)S_hi 2^32 + (double)S_lo) 2^-38).  start
    (float32[n, 3], accumulate): X = rint((double)start 2^38) for 0 <= start < 2^57, S_hi = X >> 32,
    S_lo = X & 0xffffffff; a negative or NaN start is NaN, one >= 2^57 is +inf."""
    L = np.asarray(L, dtype=np.float32).reshape(-1, 3)
    out = np.empty((len(counts), 3), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(L * np.float32(2.0 ** 19))
    assert r.dtype == np.float32
    q = 0
    for k, n in enumerate(counts):
        for c in range(3):
            lo, hi, nan, inf = 0, 0, False, False
            if start is not None:
                s = np.float64(np.float32(start[k][c]))
                if s != s or s < 0:
                    nan = True
                elif s >= 2.0 ** 57:
                    inf = True
                else:
                    X = int(np.rint(s * 2.0 ** 38))
                    hi, lo = X >> 32, X & 0xFFFFFFFF
            for x in r[q:q + n, c].tolist():
                if x != x:
                    nan = True
                elif abs(x) >= 2.0 ** 32:
                    inf = True
                elif x != 0:
                    sq = int(abs(x)) ** 2
                    lo += sq & 0xFFFFFFFF
                    hi += sq >> 32
            assert lo < 2 ** 64 and hi < 2 ** 64
            if nan:
                out[k, c] = np.nan
            elif inf:
                out[k, c] = np.inf
            else:   # (float(int) rounds to nearest even, as the device's conversion does)
                out[k, c] = np.float32((np.float64(float(hi)) * 2.0 ** 32 + np.float64(float(lo))) * 2.0 ** -38)
        q += n
    return out


def f64_sumsq(L: np.ndarray, counts, start=None) -> np.ndarray:
    """L[T, 3] float64, job k owning the next counts[k] rows -> float64[len(counts), 3]: start + L0 L0
    + L1 L1 + ..., each product rounded on its own, sequential additions in sample order."""
    L = np.asarray(L, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(counts), 3)) if start is None else np.array(start, dtype=np.float64).reshape(-1, 3).copy()
    q = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for k, n in enumerate(counts):
            acc = out[k].copy()
            for x in L[q:q + n]:
                acc = acc + x * x
            out[k] = acc
            q += n
    return out


def f64_sums(L: np.ndarray, counts, start=None) -> np.ndarray:
    """rt_render_pixels' fp64 rule: start + L0 + L1 + ..., sequential additions in sample order."""
    L = np.asarray(L, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(counts), 3)) if start is None else np.array(start, dtype=np.float64).reshape(-1, 3).copy()
    q = 0
    for k, n in enumerate(counts):
        acc = out[k].copy()
        for x in L[q:q + n]:
            acc = acc + x
        out[k] = acc
        q += n
    return out


def refine_ref(jobs: np.ndarray, sums, sumsq, rel_error, abs_floor, min_samples, max_samples, max_step):
    """rt_refine_jobs: jobs (RtPixelJob[n]), sums / sumsq [n, 3] (float32 or float64) -> (the next
    round's jobs, stats [jobs with next > 0, sum of next], margin float64[n]).  margin is |e2 - t t|
    / (t t) where the slot's answer came from that comparison (inf where it did not, or where t t
    is 0 and e2 is not): a slot with a margin of 1e-9 or less is too close to call in floating
    point."""
    n = jobs["sample_begin"].astype(np.int64) + jobs["sample_count"].astype(np.int64)
    s = np.asarray(sums).reshape(-1, 3).astype(np.float64)
    q = np.asarray(sumsq).reshape(-1, 3).astype(np.float64)
    nd = n.astype(np.float64)
    with np.errstate(all="ignore"):
        m = s / nd[:, None]
        d = q - s * m
        v = np.where(d > 0, d / (nd[:, None] - 1.0), 0.0)
        e2 = ((v[:, 0] + v[:, 1]) + v[:, 2]) / (3.0 * nd)
        mean = ((m[:, 0] + m[:, 1]) + m[:, 2]) / 3.0
        a = np.where(np.abs(mean) > abs_floor, np.abs(mean), np.float64(abs_floor))
        t = np.float64(rel_error) * a
        tt = t * t
        conv = e2 <= tt
        margin = np.where(tt > 0, np.abs(e2 - tt) / tt, np.where(e2 == tt, 0.0, np.inf))
    finite = np.isfinite(s).all(axis=1) & np.isfinite(q).all(axis=1)
    conv &= finite
    step = np.minimum(np.minimum(n, max_step), max_samples - n)
    judged = (n < max_samples) & (n >= min_samples) & finite
    nxt = np.where(n >= max_samples, 0, np.where(n < min_samples, min_samples - n, np.where(conv, 0, step)))
    out = np.zeros(len(jobs), N.RtPixelJob)
    out["pixel"] = jobs["pixel"]
    out["sample_begin"] = (n & 0xFFFFFFFF).astype(np.uint32)
    out["sample_count"] = nxt.astype(np.uint32)
    stats = np.array([int((nxt > 0).sum()), int(nxt.sum())], np.uint64)
    return out, stats, np.where(judged, margin, np.inf)
