"""rt_trace_rays / rt_trace_rays_from on spheres: every field of the fp32 hit record, per ray,
against an fp64 evaluation of the geometry -- an eps-correct closest hit (check_spheres), with
no allowance for wrong rays.  The checker sees only geometry: per (ray, sphere) the
closest-approach vector l = f + (b/a) d (f = o - c(time), a = d.d, b = -f.d) and the root pair
t = (b -+ sqrt(a (r^2 - |l|^2))) / a, evaluated in fp64 from the fp32-rounded rays and the fp64
scene -- not the device's way of writing its test.

Classification of a (ray, sphere) pair.  U = 2^-24 is the fp32 unit roundoff, m = |r| - |l| the
silhouette margin (a length): the pair is a certain miss where m < -E, can be a certain hit only
where m > E, with E a forward error bound of an fp32 evaluation of m:

  E_scene   what the scene loses on its way to fp32, measured, not bounded: |fl(c) - c| +
            time |fl(cv) - cv| + |fl(r) - r|, and U |c(time)| for the one rounding of
            c + time cv where the sphere moves.
  ordinary  E = E_scene + U (C_F |f| + C_L |l| + C_R |r|) + E_2.
            C_F = 1: f = o - c is one rounding, U |f|, of which only the part across d moves l
            to first order.  C_L = 3: the last operation that forms l rounds once, U |l|; |l|^2
            is three products and two additions, each term through at most 3 roundings: 3 U
            |l|^2, in length 1.5 U |l|; together 2.5, taken as 3.  C_R = 1: r * r is one
            rounding, in length U |r| / 2, taken as U |r|.  r^2 - |l|^2 then has the right sign
            (a difference of two floats).  E_2: b / a is wrong by at most C_B U |f| / |d| with
            C_B = 10 (b: 3 U on sum |f_i d_i| and U from f; a: 3 U; the reciprocal 2 U; the
            product U), which moves l ALONG d by e = C_B U |f| and so changes |l| only by
            sqrt(|l|^2 + e^2) - |l|.
  big       |r| >= 64 or relatively big (big_class): the kernels keep such a sphere relative to
            a near point p0 (BigF: p0 on the sphere, n = (p0 - c) / r), q = o - p0,
            b = -(q.d + r n.d), cc = |f|^2 - r^2 = q.q + 2 r n.q, disc = b^2 - a cc, and so do
            the bounds: db = C_Q U (|r| sum |n_i d_i| + sum |q_i d_i|), dcc = C_Q U (2 |r| sum
            |n_i q_i| + q.q), C_Q = 4 (q one rounding, a dot product three, the multiply-add
            one), ddisc = 2 |b| db + a dcc + 2 U (b^2 + a |cc|), and since disc / a =
            (|r| - |l|)(|r| + |l|): E = E_scene + ddisc / (a (|r| + |l|)).  They grow with |q|,
            the distance to the near point, not with |o - c|.  E_scene here is that of p0, n
            and r: |fl(p0) - p0| + |r| |fl(n) - n| + |fl(r) - r| + |r| ||fl(n)|^2 - 1| / 2
            (+ motion as above).

  tol = 1e-4 * max(1, t), the project's fp32 bound on t (test_trace_rays.py).  A root t is
  surely inside the interval where t > 0.001 + tol, surely outside where t < 0.001 - tol.
  certain miss: m < -E, or the far root surely outside.
  certain hit:  m > E and the far root surely inside; its distance is the near root where that
                is surely inside, else the far root (an upper bound of where it is hit).
  admissible roots of a pair that is no certain miss: the near root unless surely outside, the
                far root unless the near root is surely inside.  (Where r^2 < |l|^2 within E,
                both roots are taken at b / a, the closest approach.)

The sphere a ray starts on (rt_trace_rays_from, fp32): from the GIVEN origin both true roots,
t_near <= t_far.  The kernels offer t_near + t_far = 2 b / a only.  Any value between t_far and
t_near + t_far is admissible (widened by tol), never the near root; a certain hit where that
whole interval lies above 0.001 + tol (its distance: the interval's upper end), a certain miss
where it lies below 0.001 - tol; no silhouette test (the kernels make none).

A ray's answer is accepted (check_spheres) where
  * the sphere reported is no certain miss, t is within tol of an admissible root of it, and no
    sphere is certainly hit before t - tol; a miss only where nothing is certainly hit;
  * the record is that sphere's: mat exact; |p - (o + t d)| <= U (|t d| + |p|) (a product and a
    sum, or one fused rounding); the normal within E_N = (E_scene + 2 U |p - x|) / |r| + 4 U of
    +-(p - c(time)) / r (x = c, for a big sphere p0: the difference, and a division or a
    reciprocal and a product), its sign that of front_face, unit length within E_N +
    (tol |d| + U (|t d| + |p|) + off) / |r| (the point is within the t bound of the surface;
    off: on the ray's own sphere the origin's distance from it, ||f| - |r||, which the point
    at 2 b / a mirrors; in a conditioned case also the admissible ranges' widths times |d|) and,
    where |d.n| > |d| (E_N + U (|t d| + |p|) / |r| + 3 U) with n the fp64 normal at o + t d
    (the record's own p is that point rounded; the dot product three roundings), against the
    ray with front_face the fp64 sign; else the ray counts as uncertain;
  * a miss has every other field 0.

Two kinds of ray cannot meet tol by construction -- grazing rays (the roots' condition) and
short rays across the normal (2 b / a is a cancelled dot product).  Their tests stay at tol as
strict expected failures with the measured figures in their docstrings, and the same records
are checked in full as a *conditioned* case (Case(conditioned=True)): an admissible root is the
range it takes while m moves by -+E, and 2 b / a of the ray's own sphere is taken within
E_T = 2 (C_B U |f| + E_scene) / |d| -- the bounds above carried through, nothing new.

Classes (8,000 seeded rays each; references computed once and cached): field, motion, tangent,
afar, inside_* and scaled_* through rt_trace_rays; from_field, from_HOLLOW, from_SHELL,
from_ground and from_mixed (spheres and triangles) through rt_trace_rays_from, from the fp64
reference's hit points and from the device's own records, with material.h's directions."""
import numpy as np
import pytest

from raytracingproject_amd import _native as N
from raytracingproject_amd import api, rtweekend, scenes
from test_trace_mesh import as_hits, tol_of
from test_trace_rays import _rays, hollow_world, neg_field, negative_rays, shell_field, world_hit_reference

SEED = 0x5EED
TMIN = 0.001
U32 = 2.0 ** -24
C_F, C_L, C_R, C_B, C_Q = 1.0, 3.0, 1.0, 10.0, 4.0
BIG_RADIUS, BIG_RATIO, MAX_BIG = 64.0, 16.0, 8          # rt_scene.h
NRAYS = 8000


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def _norm(v):
    return np.sqrt((v * v).sum(axis=-1))


# ---- the scene as the checker sees it ----------------------------------------------------
def big_class(S):
    """Input indices of the big spheres: |r| >= BIG_RADIUS, or (rt_bvh.cpp
    relatively_big_spheres, sphere scenes) the largest of the rest while each is at least
    BIG_RATIO times the extent of the box around the spheres smaller than it."""
    r = np.abs(S["radius"])
    big = [int(k) for k in np.flatnonzero(r >= BIG_RADIUS)]
    cand = [int(k) for k in np.flatnonzero(r < BIG_RADIUS)]
    cand.sort(key=lambda k: -r[k])                      # (stable, as std::stable_sort)
    c1 = S["center"] + np.where(S["moving"][:, None] != 0, S["center_vec"], 0.0)
    lo = np.minimum(S["center"], c1) - r[:, None]
    hi = np.maximum(S["center"], c1) + r[:, None]
    room = MAX_BIG - len(big)
    rel = []
    for i, k in enumerate(cand):
        rest = cand[i + 1:]
        if len(rel) >= room or not rest:
            break
        extent = (hi[rest].max(axis=0) - lo[rest].min(axis=0)).max()
        if not (extent > 0) or not (r[k] >= BIG_RATIO * extent):
            break
        rel.append(k)
    return sorted(big + rel)


class Geo:
    """The spheres of a scene, in fp64, with what the fp32 records lose (E_scene's parts) and,
    for the big class, the near point and normal of rt_pack.cpp's BigF."""

    def __init__(self, S):
        self.S = S
        self.n = len(S)
        self.c, self.r = S["center"].astype(np.float64), S["radius"].astype(np.float64)
        self.mov = S["moving"] != 0
        self.cv = np.where(self.mov[:, None], S["center_vec"], 0.0)
        self.big = np.zeros(self.n, bool)
        self.big[big_class(S)] = True
        self.dc = _norm(_f32(self.c) - self.c)
        self.dcv = _norm(_f32(self.cv) - self.cv)
        self.dr = np.abs(_f32(self.r) - self.r)
        # BigF (rt_pack.cpp): the point of the sphere nearest the centre of the box around the
        # other spheres (static centres, |r|), the origin without others
        rest = ~self.big
        if rest.any():
            ar = np.abs(self.r[rest])[:, None]
            mid = 0.5 * ((self.c[rest] - ar).min(axis=0) + (self.c[rest] + ar).max(axis=0))
        else:
            mid = np.zeros(3)
        nv = mid[None, :] - self.c
        ln = _norm(nv)
        na = np.where((ln > 0)[:, None], nv / np.where(ln > 0, ln, 1.0)[:, None], np.array([0.0, 1.0, 0.0]))
        self.p0 = self.c + np.abs(self.r)[:, None] * na
        self.nrm = np.sign(self.r)[:, None] * na
        nf = _f32(self.nrm)
        self.dbig = (_norm(_f32(self.p0) - self.p0) + np.abs(self.r) * _norm(nf - self.nrm) + self.dr +
                     np.abs(self.r) * np.abs((nf * nf).sum(axis=1) - 1.0) / 2)


class Pairs:
    """pairs(): per (ray, sphere) -- see the module docstring."""


def pairs(g, rays, k=None, self_ids=None, rows=None, conditioned=False):
    """The geometry and classification of (ray i, sphere k[i]) (k given: one pair per ray), or of
    every sphere for the rays `rows` (k None: rays x spheres)."""
    if k is None:
        rr = rays[rows]
        o, d, tm = rr[:, None, 0:3], rr[:, None, 3:6], rr[:, None, 6]
        sel = slice(None)
        is_self = np.zeros((len(rr), g.n), bool) if self_ids is None else self_ids[rows][:, None] == np.arange(g.n)[None, :]
    else:
        o, d, tm = rays[:, 0:3], rays[:, 3:6], rays[:, 6]
        sel = k
        is_self = np.zeros(len(rays), bool) if self_ids is None else self_ids == k
    c0, cv, r, mov, big = g.c[sel], g.cv[sel], g.r[sel], g.mov[sel], g.big[sel]
    ar = np.abs(r)
    tmx = tm[..., None]
    cen = c0 + tmx * cv
    f = o - cen
    a = (d * d).sum(axis=-1)
    dl = np.sqrt(a)
    b = -(f * d).sum(axis=-1)
    l = f + (b / a)[..., None] * d
    nl, nf = _norm(l), _norm(f)
    m = ar - nl
    with np.errstate(invalid="ignore", divide="ignore"):
        # the root pair (the stable form: c / q and q / a); r^2 < |l|^2: both at b / a
        disc = np.maximum(ar * ar - nl * nl, 0.0)
        q = b + np.copysign(np.sqrt(a * disc), b)
        cc = (nf - ar) * (nf + ar)
        ta, tb = np.where(q != 0, cc / np.where(q != 0, q, 1.0), 0.0), q / a
        ta = np.where(m < 0, b / a, ta)
        tb = np.where(m < 0, b / a, tb)
    t1, t2 = np.minimum(ta, tb), np.maximum(ta, tb)
    # E
    e_motion = np.where(mov, U32 * _norm(cen), 0.0)
    e_scene = g.dc[sel] + np.abs(tm) * g.dcv[sel] + g.dr[sel] + e_motion
    e_along = C_B * U32 * nf
    e_ord = e_scene + U32 * (C_F * nf + C_L * nl + C_R * ar) + (np.sqrt(nl * nl + e_along * e_along) - nl)
    p0 = g.p0[sel] + tmx * cv
    nn = g.nrm[sel]
    qv = o - p0
    db = C_Q * U32 * (ar * (np.abs(nn * d)).sum(axis=-1) + np.abs(qv * d).sum(axis=-1))
    dcc = C_Q * U32 * (2 * ar * np.abs(nn * qv).sum(axis=-1) + (qv * qv).sum(axis=-1))
    ddisc = 2 * np.abs(b) * db + a * dcc + 2 * U32 * (b * b + a * np.abs(cc))
    e_big_scene = g.dbig[sel] + np.abs(tm) * g.dcv[sel] + np.where(mov, U32 * _norm(p0), 0.0)
    e_big = e_big_scene + ddisc / (a * (ar + nl))
    E = np.where(big, e_big, e_ord)
    P = Pairs()
    P.e_scene = np.where(big, e_big_scene, e_scene)
    P.ref_point = np.where(np.asarray(big)[..., None], p0, cen)
    P.cen = cen

    def sure_in(t):
        return t > TMIN + tol_of(t)

    def sure_out(t):
        return t < TMIN - tol_of(t)
    # the admissible roots as ranges [lo, hi]: the roots themselves, or (conditioned) all they
    # can be while the margin moves by -+E -- where a ray grazes, by up to sqrt(2 |r| E) / |d|
    lo1, hi1, lo2, hi2 = t1, t1, t2, t2
    # the ray's own sphere: between t_far and t_near + t_far = 2 b / a; conditioned: 2 b / a as
    # fp32 can deliver it, wrong by up to E_T = 2 (C_B U |f| + E_scene) / |d| (E_2's bound of
    # b / a and the centre's error along d; big: db / a in place of C_B U |f| / |d|) -- for a
    # short direction across the normal, b is what cancellation leaves of |f| |d|
    s_lo, s_hi = np.minimum(t2, t1 + t2), np.maximum(t2, t1 + t2)
    if conditioned:
        with np.errstate(invalid="ignore"):
            sp = np.sqrt(a * np.maximum((ar + E) ** 2 - nl * nl, 0.0))
            sm = np.sqrt(a * np.maximum(np.maximum(ar - E, 0.0) ** 2 - nl * nl, 0.0))
        lo1, hi1 = np.minimum((b - sp) / a, t1), np.maximum((b - sm) / a, t1)
        lo2, hi2 = np.minimum((b + sm) / a, t2), np.maximum((b + sp) / a, t2)
        e_t = 2 * np.where(big, db / a + e_big_scene / dl, (C_B * U32 * nf + e_scene) / dl)
        s_lo, s_hi = s_lo - e_t, s_hi + e_t
    # not the ray's own sphere
    cmiss = (m < -E) | sure_out(hi2)
    chit = (m > E) & sure_in(lo2)
    chit_t = np.where(sure_in(lo1), hi1, hi2)
    adm1, adm2 = ~sure_out(hi1), ~sure_in(lo1)
    clean = chit & (sure_in(lo1) | sure_out(hi1))
    exact = np.where(t1 > TMIN, t1, np.where(t2 > TMIN, t2, np.inf))
    exact = np.where(nl <= ar, exact, np.inf)
    s_hit, s_miss = sure_in(s_lo) & sure_in(s_hi), sure_out(s_lo) & sure_out(s_hi)
    P.cmiss = np.where(is_self, s_miss, cmiss)
    P.chit = np.where(is_self, s_hit, chit)
    P.chit_t = np.where(is_self, s_hi, chit_t)
    P.clean = np.where(is_self, s_hit, clean)
    P.adm1, P.adm2 = np.where(is_self, True, adm1), np.where(is_self, False, adm2)
    P.lo1, P.hi1 = np.where(is_self, s_lo, lo1), np.where(is_self, s_hi, hi1)
    P.lo2, P.hi2 = lo2, hi2
    # how far the point of an admissible t can lie off the sphere: the origin's own distance for
    # the ray's own sphere (the point at 2 b / a mirrors the origin), and the ranges' widths
    P.off = np.where(is_self, np.abs(nf - ar) + (s_hi - s_lo - np.abs(t1)) * dl, np.maximum(hi1 - lo1, hi2 - lo2) * dl)
    P.first = np.where(P.adm1, P.lo1, P.lo2)          # the earliest admissible root
    P.exact = np.where(is_self, np.where(t2 > TMIN, t2, np.inf), exact)
    P.exact_noself = exact
    P.is_self = is_self
    return P


def record_of(g, rays, k, t):
    """sphere::hit's record of ray i on sphere k[i] at t[i], fp64: p, normal, front -- p as fp32
    holds it, the normal from that p (as any fp32 record's is)."""
    o, d, tm = rays[:, 0:3], rays[:, 3:6], rays[:, 6]
    p = _f32(o + t[:, None] * d)
    outward = (p - (g.c[k] + tm[:, None] * g.cv[k])) / g.r[k][:, None]
    front = (d * outward).sum(axis=1) < 0
    return p, np.where(front[:, None], outward, -outward), front


class Case:
    """A ray class on a sphere scene: the rays rounded to fp32 (so that only the arithmetic
    differs from the device), self_ids (None: rt_trace_rays), and per ray, from the geometry
    alone: tstar, the smallest certain-hit distance (inf: none); whether every sphere is a
    certain miss; ambiguous (a candidate that is neither a certain miss nor a clean certain hit
    could precede tstar + tol); tied (two certain hits within 2 tol); the exact closest and
    second-closest spheres under the self rule, and the exact closest sphere without it."""

    def __init__(self, S, M, rays, self_ids=None, kind=None, kinds=("all",), conditioned=False, chunk=256):
        self.S, self.M, self.g = S, M, Geo(S)
        self.conditioned = conditioned      # (pairs: the roots as the ranges fp32 can deliver)
        self.rays = _f32(rays)
        n = len(rays)
        self.self_ids = None if self_ids is None else np.asarray(self_ids, dtype=np.int64)
        self.kind = np.zeros(n, int) if kind is None else kind
        self.kinds = list(kinds)
        self.tstar, self.all_miss = np.empty(n), np.empty(n, bool)
        self.ambiguous, self.tied = np.empty(n, bool), np.empty(n, bool)
        self.id1, self.t1, self.id2, self.t2 = np.empty(n, int), np.empty(n), np.empty(n, int), np.empty(n)
        self.id_noself = np.empty(n, int)
        for s in range(0, n, chunk):
            rows = np.arange(s, min(n, s + chunk))
            P = pairs(self.g, self.rays, None, self.self_ids, rows, conditioned)
            ct = np.where(P.chit, P.chit_t, np.inf)
            ts = ct.min(axis=1)
            self.tstar[rows] = ts
            self.all_miss[rows] = P.cmiss.all(axis=1)
            lim = np.where(np.isfinite(ts), ts + tol_of(ts), np.inf)[:, None]
            self.ambiguous[rows] = (~P.cmiss & ~P.clean & (P.first < lim)).any(axis=1)
            lim2 = np.where(np.isfinite(ts), ts + 2 * tol_of(ts), -np.inf)[:, None]
            self.tied[rows] = (ct <= lim2).sum(axis=1) >= 2
            order = np.argsort(P.exact, axis=1)[:, :2]
            rr = np.arange(len(rows))
            self.id1[rows], self.id2[rows] = order[:, 0], order[:, 1]
            self.t1[rows], self.t2[rows] = P.exact[rr, order[:, 0]], P.exact[rr, order[:, 1]]
            k0 = P.exact_noself.argmin(axis=1)
            self.id_noself[rows] = np.where(np.isfinite(P.exact_noself[rr, k0]), k0, -1)
        self.id1 = np.where(np.isfinite(self.t1), self.id1, -1)
        self.id2 = np.where(np.isfinite(self.t2), self.id2, -1)
        self.certain_hit = np.isfinite(self.tstar) & ~self.ambiguous
        self.certain_miss = self.all_miss

    def reference_hits(self):
        """The fp64 closest hit under the self rule as HIT_DTYPE records, rounded to fp32."""
        hit = self.id1 >= 0
        k = np.maximum(self.id1, 0)
        t = _f32(np.where(hit, self.t1, 0.0))
        p, nrm, front = record_of(self.g, self.rays, k, t)
        z = ~hit
        h = as_hits(t, _f32(np.where(z[:, None], 0.0, p)), _f32(np.where(z[:, None], 0.0, nrm)), front & hit,
                    self.id1, np.where(hit, self.S["mat"][k], 0))
        return h

    def shares(self, mask):
        return {k: float(mask[self.kind == i].mean()) for i, k in enumerate(self.kinds)}


def check_spheres(c, h):
    """-> (why, ratios): why[i] is '' where ray i's record passes, else the first rule it breaks
    (module docstring); ratios: the largest error over its bound of t, p and the normal among
    the rays that pass.  A conditioned case (Case(conditioned=True)) takes an admissible root
    for the whole range it has while the margin m moves by -+E, and 2 b / a of the ray's own
    sphere within E_T (pairs): the same bounds carried through the roots' own condition, which
    for grazing rays and for short directions across the normal exceeds tol."""
    n, g = len(c.rays), c.g
    o, d = c.rays[:, 0:3], c.rays[:, 3:6]
    why = np.full(n, "", dtype=object)

    def flag(mask, msg):
        why[mask & (why == "")] = msg
    ids = h["id"].astype(np.int64)
    t = h["t"].astype(np.float64)
    flag((ids < -1) | (ids >= g.n), "id out of range")
    miss = ids == -1
    sph = (ids >= 0) & (ids < g.n)
    flag(miss & np.isfinite(c.tstar), "a miss, but a sphere is certainly hit")
    zero = (t == 0) & (h["p"] == 0).all(axis=1) & (h["normal"] == 0).all(axis=1) & (h["front_face"] == 0) & (h["mat"] == 0)
    flag(miss & ~zero, "a miss with a field that is not 0")
    k = np.clip(ids, 0, g.n - 1)
    P = pairs(g, c.rays, k, c.self_ids, conditioned=c.conditioned)
    flag(sph & P.cmiss, "a sphere the ray certainly misses")
    lo1, hi1, lo2, hi2 = P.lo1, P.hi1, P.lo2, P.hi2
    with np.errstate(invalid="ignore"):
        in1 = P.adm1 & (t >= lo1 - tol_of(lo1)) & (t <= hi1 + tol_of(hi1))
        in2 = P.adm2 & (t >= lo2 - tol_of(lo2)) & (t <= hi2 + tol_of(hi2))
        # (error over bound: against the nearer admissible interval)
        e1 = np.maximum(lo1 - t, t - hi1) / np.where(t < lo1, tol_of(lo1), tol_of(hi1))
        e2 = np.maximum(lo2 - t, t - hi2) / np.where(t < lo2, tol_of(lo2), tol_of(hi2))
    rt = np.maximum(np.minimum(np.where(P.adm1, e1, np.inf), np.where(P.adm2, e2, np.inf)), 0.0)
    flag(sph & ~(in1 | in2), "t")
    flag(sph & (c.tstar < t - tol_of(t)), "not the closest hit")
    flag(sph & (h["mat"] != c.S["mat"][k]), "mat")
    # the record
    td = t[:, None] * d
    p64 = o + td
    p_bound = U32 * (_norm(td) + _norm(p64))
    perr = _norm(h["p"] - p64)
    flag(sph & ~(perr <= p_bound), "p")
    ar = np.abs(g.r[k])
    e_n = (P.e_scene + 2 * U32 * _norm(h["p"] - P.ref_point)) / ar + 4 * U32
    outward = (h["p"] - P.cen) / g.r[k][:, None]
    sgn = np.where(h["front_face"] != 0, 1.0, -1.0)[:, None]
    nerr = _norm(h["normal"] - sgn * outward)
    flag(sph & ~(nerr <= e_n), "normal")
    unit_bound = e_n + (tol_of(t) * _norm(d) + p_bound + P.off) / ar
    flag(sph & ~(np.abs(_norm(h["normal"]) - 1.0) <= unit_bound), "normal is not of unit length")
    out64 = (p64 - P.cen) / g.r[k][:, None]
    dn = (d * out64).sum(axis=1)
    sure = np.abs(dn) > _norm(d) * (e_n + p_bound / ar + 3 * U32)
    flag(sph & sure & ~((h["normal"] * d).sum(axis=1) < 0), "normal does not face the ray")
    flag(sph & sure & ((h["front_face"] != 0) != (dn < 0)), "front_face")
    ok = sph & (why == "")
    with np.errstate(invalid="ignore", divide="ignore"):
        ratios = {"t": float(rt[ok].max(initial=0.0)),
                  "p": float((perr[ok] / p_bound[ok]).max(initial=0.0)),
                  "normal": float((nerr[ok] / e_n[ok]).max(initial=0.0))}
    c.face_uncertain = sph & ~sure
    return why, ratios


def _summary(why):
    u, cnt = np.unique(why[why != ""], return_counts=True)
    return dict(zip(u.tolist(), cnt.tolist()))


# ---- scenes ------------------------------------------------------------------------------
_WORLD = {}


def field():
    if "field" not in _WORLD:
        rtweekend.reset_stream()
        _WORLD["field"] = api.flatten(scenes.random_spheres())
    return _WORLD["field"]


def scene(name):
    """(S, M) of a test scene."""
    if name == "field":
        return field()
    if name not in _WORLD:
        S, M = field()
        if name == "NEG":
            S = neg_field(S)
        elif name == "NEG_GROUND":
            S = neg_field(S, ground=True)
        elif name == "SHELL":
            S = shell_field(S, M)
        elif name == "HOLLOW":
            S, M = hollow_world()
        elif name == "motion":
            # test_sphere_grid_time_slabs_with_motion_on_every_axis (test_gpu_parity.py)
            S = S.copy()
            g = np.random.default_rng(7)
            small = S["radius"] < 0.5
            S["moving"][small] = 1
            S["center_vec"][small] = g.uniform(-0.6, 0.6, (int(small.sum()), 3))
        elif name == "ground":
            # the field and a second, moving member of the big class behind it
            S = np.concatenate([S, S[-1:]])
            S[-1]["center"], S[-1]["radius"], S[-1]["moving"] = (0.0, 60.0, -220.0), 100.0, 1
            S[-1]["center_vec"] = (3.0, 5.0, -2.0)
        elif name in SCALED:
            scale, shift = SCALED[name]
            S = S.copy()
            S["center"] = S["center"] * scale + np.array(shift)
            S["center_vec"] = S["center_vec"] * scale
            S["radius"] = S["radius"] * scale
        else:
            raise ValueError(name)
        _WORLD[name] = (S, M)
    return _WORLD[name]


SCALED = {"x100_shifted": (100.0, (1.0e4, 0.0, -1.0e4)), "x1e-3": (1.0e-3, (0.0, 0.0, 0.0))}


# ---- rays without origin ids -------------------------------------------------------------
def _join(o, d, tm):
    return np.concatenate([o, d, np.broadcast_to(tm, (len(o), 1))], axis=1)


def _unit(v):
    return v / _norm(v)[:, None]


def _centres(S, k, tm):
    return S["center"][k] + np.where(S["moving"][k][:, None] != 0, tm * S["center_vec"][k], 0.0)


def tangent_rays(S, n, seed):
    """Aimed at silhouettes: the impact parameter on the target is |r| (1 +- 10^-k), k = 2..7.
    Three quarters at the field's spheres, from 3 to 15 radii away and below the centre, at the
    upper half of the silhouette -- a ray that passes outside it climbs over the field into the
    sky; a quarter at the ground from origins up to 900 away from its top, 0.05 to 5 above it."""
    g = np.random.default_rng(seed)
    nb = n // 4
    ns = n - nb
    k = np.concatenate([g.integers(1, len(S), ns), np.zeros(nb, int)])
    tm = g.uniform(0, 1, (n, 1))
    c = _centres(S, k, tm)
    r = np.abs(S["radius"][k])
    phi = g.uniform(0, 2 * np.pi, ns)
    o = c.copy()
    o[:ns] += np.stack([np.cos(phi), np.zeros(ns), np.sin(phi)], axis=1) * (r[:ns] * g.uniform(3, 15, ns))[:, None]
    o[:ns, 1] = g.uniform(0.02, 1.0, ns) * c[:ns, 1]
    az = g.uniform(0, 2 * np.pi, nb)
    xz = np.stack([np.cos(az), np.sin(az)], axis=1) * g.uniform(0, 900, (nb, 1))
    up =np.sqrt(1000.0 ** 2 - (xz * xz).sum(axis=1)) - 1000.0
    o[ns:] = np.stack([xz[:, 0], up + g.uniform(0.05, 5.0, nb), xz[:, 1]], axis=1)
    f = c - o
    D = _norm(f)
    u = f / D[:, None]
    # the silhouette point's direction across the ray: straight up turned by up to 60 degrees
    # about the line to the centre (the ground: any)
    top = _unit(np.array([0.0, 1.0, 0.0]) - u[:, 1:2] * u)
    side = np.cross(u, top)
    turn = np.concatenate([g.uniform(-np.pi / 3, np.pi / 3, ns), g.uniform(-np.pi, np.pi, nb)])
    w = top * np.cos(turn)[:, None] + side * np.sin(turn)[:, None]
    impact = r * (1.0 + g.choice([-1.0, 1.0], n) * 10.0 ** -g.integers(2, 8, n).astype(float))
    sin = np.minimum(impact / D, 1.0)
    d = (u * np.sqrt(1.0 - sin * sin)[:, None] + w * sin[:, None]) * (D * g.uniform(0.05, 2.0, n))[:, None]
    return _join(o, d, tm), np.concatenate([np.zeros(ns, int), np.ones(nb, int)]), ["spheres", "ground"]


def afar_rays(S, n, seed):
    """The field's spheres seen from 1e3 to 1e4 away, |d| from 1e-3 to 1e3.  tol is 1e-4 of the
    distance here, 0.1 to 1: two spheres a ray meets that close together tie, and so would any
    sphere with the ground behind it.  So the rays run level, at least 0.42 above the ground's
    top -- over the static small spheres (tops at 0.4) -- aimed within two radii of the centres
    of the spheres that reach above 0.5 at the ray's time (the three of R = 1 and the moving
    ones); those that meet nothing pass over the ground's curve."""
    g = np.random.default_rng(seed)
    tm = g.uniform(0, 1, (n, 1))
    top = S["center"][None, 1:, 1] + np.where(S["moving"][None, 1:] != 0, tm * S["center_vec"][None, 1:, 1], 0.0) + \
        np.abs(S["radius"][None, 1:])
    k = 1 + (g.random(top.shape) * (top > 0.5)).argmax(axis=1)      # one of the high ones, at random
    c = _centres(S, k, tm)
    r = np.abs(S["radius"][k])
    phi = g.uniform(0, 2 * np.pi, n)
    away = np.stack([np.cos(phi), np.zeros(n), np.sin(phi)], axis=1)
    off = _unit(np.cross(away, g.normal(size=(n, 3))))
    aim = c + off * (r * g.uniform(0, 2, n))[:, None]
    aim[:, 1] = np.maximum(aim[:, 1], 0.42)
    dist = 10.0 ** g.uniform(3, 4, n)
    o = aim + away * dist[:, None]
    d = _unit(aim - o) * (10.0 ** g.uniform(-3, 3, n))[:, None]
    return _join(o, d, tm), (dist > 10.0 ** 3.5).astype(int), ["1e3 - 3e3", "3e3 - 1e4"]


def inside_rays(S, which, n, seed):
    """Origins well inside the spheres `which` (within half the radius of the centre at the
    ray's time), in every direction."""
    g = np.random.default_rng(seed)
    k = which[g.integers(0, len(which), n)]
    tm = g.uniform(0, 1, (n, 1))
    off = _unit(g.normal(size=(n, 3))) * (0.5 * np.abs(S["radius"][k]) * g.uniform(0, 1, n))[:, None]
    d = g.normal(size=(n, 3)) * g.uniform(0.05, 2.0, (n, 1))
    return _join(_centres(S, k, tm) + off, d, tm)


INSIDE = ["field", "NEG", "SHELL", "HOLLOW", "NEG_GROUND"]
PLAIN = (["field", "motion", "tangent", "afar"] + ["inside_" + s for s in INSIDE] + ["scaled_" + s for s in SCALED])
CAN_MISS = {"field", "motion", "tangent", "afar", "scaled_x100_shifted", "scaled_x1e-3"}


def plain_case(name):
    """-> (scene name, rays, kind, kinds) of a class without origin ids."""
    if name == "field":
        return "field", _rays(NRAYS), None, ("all",)
    if name == "motion":
        rays = _rays(NRAYS, seed=3)
        rays[:, 6] = np.array([0.0, 0.5, float(np.nextafter(np.float32(1), np.float32(0)))])[np.arange(NRAYS) % 3]
        return "motion", rays, np.arange(NRAYS) % 3, ("time 0", "time 0.5", "time 1-")
    if name == "tangent":
        return ("field",) + tuple(tangent_rays(field()[0], NRAYS, 4))
    if name == "afar":
        # (with tol up to a unit of length, 7 % of these rays meet two spheres within 2 tol: the
        # class keeps the first NRAYS of a larger draw that the reference does not call tied)
        S, M = field()
        rays, kind, kinds = afar_rays(S, NRAYS + NRAYS // 8, 5)
        keep = np.flatnonzero(~Case(S, M, rays).tied)[:NRAYS]
        assert len(keep) == NRAYS
        return "field", rays[keep], kind[keep], kinds
    if name.startswith("inside_"):
        sn = name[len("inside_"):]
        S, M = scene(sn)
        if sn == "field":
            which = np.flatnonzero(M["type"][S["mat"]] == N.RT_DIELECTRIC)
        else:
            which = np.flatnonzero(S["radius"] < 0)
        return sn, inside_rays(S, which, NRAYS // len(INSIDE), 6), None, ("all",)
    if name.startswith("scaled_"):
        # the field and its rays scaled together, so t -- and with it tmin and tol -- is the
        # unscaled scene's
        scale, shift = SCALED[name[len("scaled_"):]]
        rays = _rays(NRAYS, seed=7)
        rays[:, 0:3] = rays[:, 0:3] * scale + np.array(shift)
        rays[:, 3:6] *= scale
        return name[len("scaled_"):], rays, None, ("all",)
    raise ValueError(name)


# ---- rays that start on a primitive (material.h's directions) -----------------------------
def _random_unit(g, n):
    return _unit(g.normal(size=(n, 3)))


def _reflect(v, nrm):
    return v - 2 * (v * nrm).sum(axis=1)[:, None] * nrm                       # vec3.h reflect


def scatter_dirs(kind, g, d_in, nrm, front):
    """The directions material.h gives a ray that arrives along d_in at a point with normal nrm
    (against the ray) -> d.
    lambert  normal + unit vector (material.h:19-25);
    short    the same with the unit vector within 1e-6 .. 1e-2 of -normal, so |d| is that short;
    metal    reflect(unit(d_in), normal) + fuzz * unit vector, fuzz 0, 0.3 and 1 by thirds;
    refract_in, refract_out, tir
             dielectric ir 1.5 (material.h:54-70): ratio 1/1.5 into a front face, 1.5 out of a
             back face, reflected where ratio * sin > 1 (total internal reflection)."""
    n = len(nrm)
    if kind == "lambert":
        return nrm + _random_unit(g, n)
    if kind == "short":
        w = _unit(np.cross(nrm, g.normal(size=(n, 3))))
        delta = 10.0 ** g.uniform(-6, -2, n)
        u = _unit(-nrm + delta[:, None] * w)
        return nrm + u
    uv = _unit(d_in)
    if kind == "metal":
        fuzz = np.array([0.0, 0.3, 1.0])[np.arange(n) % 3]
        return _reflect(uv, nrm) + fuzz[:, None] * _random_unit(g, n)
    if kind in ("refract_in", "refract_out", "tir"):
        ratio = np.where(front, 1.0 / 1.5, 1.5)
        cos = np.minimum(-(uv * nrm).sum(axis=1), 1.0)
        sin = np.sqrt(1.0 - cos * cos)
        perp = ratio[:, None] * (uv + cos[:, None] * nrm)
        par = -np.sqrt(np.abs(1.0 - (perp * perp).sum(axis=1)))[:, None] * nrm
        return np.where((ratio * sin > 1.0)[:, None], _reflect(uv, nrm), perp + par)
    raise ValueError(kind)


def _cannot_refract(d_in, nrm):
    cos = np.minimum(-(_unit(d_in) * nrm).sum(axis=1), 1.0)
    return 1.5 * np.sqrt(1.0 - cos * cos) > 1.0


# kind -> its share of a class's rays.  The short rays are a tenth: where fp32 rounding put
# their origin inside its sphere, the ray's true exit root is admissible beside 2 b / a, so the
# ray is ambiguous by construction (about a quarter of them on the field, more on the ground).
KINDS = {"lambert": 0.2, "short": 0.1, "metal": 0.3, "refract_in": 0.15, "refract_out": 0.15, "tir": 0.1}


def first_batch(sn, seed=11):
    """The rays whose hit points start the from_* rays: camera and interior rays and, so that
    back faces are hit from inside, rays that start within spheres."""
    S, M = scene(sn)
    if sn in ("SHELL", "HOLLOW"):
        return negative_rays(S, NRAYS, seed)
    inner = inside_rays(S, np.arange(1, len(S)), NRAYS // 2, seed + 1)
    return np.concatenate([_rays(NRAYS, seed), inner])


def scattered(first, p, nrm, front, ids, keep, kinds, n, seed):
    """n rays from the hit points (p, nrm, front, ids) of `first` where keep, the kinds by their
    shares, each from the hit points it applies to (refract_in: front faces; refract_out and
    tir: back faces that can and cannot refract; a scene without such hits: any)
    -> (rays, origin ids, kind index)."""
    g = np.random.default_rng(seed)
    names = list(kinds)
    kind = np.repeat(np.arange(len(names)), [int(round(n * kinds[k])) for k in names])[:n]
    kind = np.concatenate([kind, np.zeros(n - len(kind), int)])
    tir = _cannot_refract(first[:, 3:6], nrm)
    applies = {"refract_in": front, "refract_out": ~front & ~tir, "tir": ~front & tir}
    o, d, oid, tm = np.empty((n, 3)), np.empty((n, 3)), np.empty(n, int), np.empty((n, 1))
    for i, kd in enumerate(names):
        ok = np.flatnonzero(keep & applies.get(kd, True))
        if len(ok) < 100:
            ok = np.flatnonzero(keep)
        assert len(ok) >= 100, (kd, len(ok))
        w = kind == i
        q = ok[g.integers(0, len(ok), int(w.sum()))]
        d[w] = scatter_dirs(kd, g, first[q, 3:6], nrm[q], front[q])
        o[w], oid[w], tm[w] = p[q], ids[q], first[q, 6:7]
    return _join(o, d, tm), oid, kind


FROM = ["from_field", "from_HOLLOW", "from_SHELL", "from_ground"]
FROM_SCENE = {"from_field": "field", "from_HOLLOW": "HOLLOW", "from_SHELL": "SHELL", "from_ground": "ground",
              "short": "field"}


def from_case(name, device_hits=None):
    """-> (scene name, rays, origin ids, kind, kinds) of a class of rays that start on spheres:
    at the fp64 reference's hit points of first_batch (rounded to fp32 with the rays), or at the
    device's own fp32 records of it (device_hits).  from_ground starts on the big spheres only,
    the others on every sphere but the ground; `short` is from_field's short kind alone."""
    sn = FROM_SCENE[name]
    S, M = scene(sn)
    first = _f32(first_batch(sn))
    if device_hits is None:
        _, p, nrm, front, ids = world_hit_reference(S, M, first)
    else:
        p, nrm, front, ids = device_hits["p"], device_hits["normal"], device_hits["front_face"] != 0, device_hits["id"]
    on_big = Geo(S).big[np.maximum(ids, 0)]
    keep = (ids >= 0) & (on_big if name == "from_ground" else ~on_big)
    kinds = {"short": 1.0} if name == "short" else KINDS
    rays, oid, kind = scattered(first, p, nrm, front, ids, keep, kinds, NRAYS, 12)
    return sn, rays, oid, kind, list(kinds)


_CASES = {}


def case(name):
    if name not in _CASES:
        if name in PLAIN:
            sn, rays, kind, kinds = plain_case(name)
            oid = None
        else:
            sn, rays, oid, kind, kinds = from_case(name)
        _CASES[name] = (sn, Case(*scene(sn), rays, oid, kind, kinds))
    return _CASES[name]


# ---- CPU tests ---------------------------------------------------------------------------
def test_big_class_of_the_scenes():
    """The restated big class: the ground alone on the field at either small scale, the ground
    and the three R = 100 spheres at x100, the added moving sphere on `ground`."""
    assert big_class(field()[0]) == [0]
    assert big_class(scene("x1e-3")[0]) == [0]
    S100 = scene("x100_shifted")[0]
    assert big_class(S100) == sorted(np.flatnonzero(np.abs(S100["radius"]) >= 64).tolist()) and len(big_class(S100)) == 4
    assert big_class(scene("ground")[0]) == [0, len(field()[0])]
    assert big_class(scene("HOLLOW")[0]) == [0] and big_class(scene("NEG_GROUND")[0]) == [0]


def test_pairs_agree_with_the_list_order_reference():
    """The geometry's exact closest sphere is world_hit_reference's (the reference's operation
    order) on the field's rays: the same id, t within 1e-9 max(1, t)."""
    sn, c = case("field")
    t, _, _, _, ids = world_hit_reference(c.S, c.M, c.rays)
    assert np.array_equal(c.id1, ids) and np.array_equal(c.id_noself, ids)
    hit = ids >= 0
    assert np.all(np.abs(c.t1[hit] - t[hit]) <= 1e-9 * np.maximum(1.0, t[hit]))


@pytest.mark.parametrize("name", PLAIN + FROM)
def test_class_caps(name):
    """From the reference alone, per class: ambiguous rays at most 5 % (tangent: instead at
    least 25 % certain hits and 25 % certain misses), rays with two certain hits within 2 tol at
    most 1 %, certain hits at least 25 %, certain misses at least 5 % where the class can miss;
    and the checker accepts the fp64 reference's own records rounded to fp32."""
    sn, c = case(name)
    amb, tied = float(c.ambiguous.mean()), float(c.tied.mean())
    chit, cmiss = float(c.certain_hit.mean()), float(c.certain_miss.mean())
    print(name, "certain hit %.4f certain miss %.4f ambiguous %.4f tied %.4f" % (chit, cmiss, amb, tied),
          "by kind: ambiguous", c.shares(c.ambiguous), "certain hit", c.shares(c.certain_hit))
    if name == "tangent":
        assert cmiss >= 0.25
    else:
        assert amb <= 0.05, amb
    assert tied <= 0.01, tied
    assert chit >= 0.25, chit
    if name in CAN_MISS or name in FROM:
        assert cmiss >= 0.05, cmiss
    why, ratios = check_spheres(c, c.reference_hits())
    print(name, "reference records: error over bound", ratios)
    assert not (why != "").any(), _summary(why)


def test_short_rays_need_the_self_rule():
    """The premise of rt_trace_rays_from: on the short Lambertian rays the exact fp64 closest
    sphere with and without the self rule differs on at least 5 % of rays (fp32-rounded hit
    points lie off their sphere, and |d| << 1 puts the false root above tmin)."""
    sn, c = case("short")
    differ = float((c.id1 != c.id_noself).mean())
    print("short rays: closest sphere differs on", differ, "hit with", float((c.id1 >= 0).mean()),
          "without", float((c.id_noself >= 0).mean()))
    assert differ >= 0.05, differ


def test_checker_rejects_mutations():
    """check_spheres accepts the reference's records and rejects each way of being subtly wrong,
    on the rays where that way differs by more than the rule allows."""
    sn, c = case("field")
    g = c.g
    ref = c.reference_hits()
    why, _ = check_spheres(c, ref)
    assert not (why != "").any(), _summary(why)
    n = len(ref)
    hit = ref["id"] >= 0
    k1 = np.maximum(c.id1, 0)
    P1 = pairs(g, c.rays, k1)
    clear = hit & ~c.ambiguous & P1.clean & ~c.face_uncertain
    assert clear.mean() > 0.3

    def mutate(**f):
        h = ref.copy()
        for name, v in f.items():
            h[name] = v
        return h

    def rejected(h, where, cause=None):
        assert where.sum() > 100, int(where.sum())
        w, _ = check_spheres(c, h)
        assert (w[where] != "").all(), (int((w[where] == "").sum()), int(where.sum()))
        if cause is not None:
            assert set(_summary(w[where])) <= set(cause), _summary(w[where])
    # the second-closest sphere, with its own (correct) record
    has2 = clear & (c.id2 >= 0) & (c.t2 > c.t1 + 3 * tol_of(c.t2))
    k2 = np.maximum(c.id2, 0)
    t2 = np.where(has2, c.t2, 0.0)
    p2, n2, f2 = record_of(g, c.rays, k2, t2)
    h = ref.copy()
    w2 = has2
    h["t"][w2], h["p"][w2], h["normal"][w2] = _f32(t2[w2]), _f32(p2[w2]), _f32(n2[w2])
    h["front_face"][w2], h["id"][w2], h["mat"][w2] = f2[w2], k2[w2], c.S["mat"][k2[w2]]
    rejected(h, has2, {"not the closest hit"})
    # t scaled by 1 +- 3e-4, p and the normal moved with it (beyond tol where t > 1)
    for s in (1 + 3e-4, 1 - 3e-4):
        ts = _f32(ref["t"] * s)
        ps, ns, fs = record_of(g, c.rays, k1, ts)
        rejected(mutate(t=ts, p=_f32(ps), normal=_f32(ns)), clear & (ref["t"] > 1.0), {"t"})
    # the far root where the near one is certain
    far = clear & (P1.lo2 > P1.lo1 + 3 * tol_of(P1.lo2)) & (np.abs(ref["t"] - P1.lo1) <= tol_of(P1.lo1))
    pf, nf_, ff = record_of(g, c.rays, k1, P1.lo2)
    h = ref.copy()
    h["t"][far], h["p"][far], h["normal"][far], h["front_face"][far] = (_f32(P1.lo2[far]), _f32(pf[far]), _f32(nf_[far]),
                                                                       ff[far])
    rejected(h, far, {"t"})
    # every id shifted by one (the record otherwise unchanged)
    rejected(mutate(id=np.where(hit, (ref["id"] + 1) % g.n, -1)), clear)
    # the normal negated; front_face flipped; both
    rejected(mutate(normal=-ref["normal"]), clear, {"normal"})
    rejected(mutate(front_face=1 - ref["front_face"]), clear, {"normal"})
    rejected(mutate(normal=-ref["normal"], front_face=1 - ref["front_face"]), clear,
             {"normal does not face the ray", "front_face"})
    # the material of another sphere
    rejected(mutate(mat=(ref["mat"] + 1) % len(c.M)), clear, {"mat"})
    # p moved along the ray by 1e-5 of its distance (the bound is 2^-24-relative)
    rejected(mutate(p=ref["p"] + 1e-5 * (ref["p"] - c.rays[:, 0:3])), clear & (ref["t"] > 0.1), {"p", "normal"})
    # a hit turned into a miss
    h = ref.copy()
    h[clear] = np.zeros(1, N.HIT_DTYPE)
    h["id"][clear] = -1
    rejected(h, clear, {"a miss, but a sphere is certainly hit"})
    # a miss turned into a hit on the sphere whose closest approach is nearest
    gone = c.certain_miss
    h = ref.copy()
    kk = np.full(n, 1)
    tt = np.full(n, 5.0)
    pm, nm, fm = record_of(g, c.rays, kk, tt)
    h["t"][gone], h["p"][gone], h["normal"][gone] = 5.0, _f32(pm[gone]), _f32(nm[gone])
    h["front_face"][gone], h["id"][gone], h["mat"][gone] = fm[gone], 1, c.S["mat"][1]
    rejected(h, gone, {"a sphere the ray certainly misses"})
    # a miss with a stale field
    h = ref.copy()
    h["mat"][gone] = 1
    rejected(h, gone, {"a miss with a field that is not 0"})


def test_checker_rejects_the_near_root_on_the_origin_sphere():
    """Rays that start on a sphere and enter it (refraction): the far root is accepted, the
    near root -- the origin itself, as a test without the self rule reports it where rounding
    lifts it above tmin -- is not."""
    sn, c = case("from_field")
    ref = c.reference_hits()
    why, _ = check_spheres(c, ref)
    assert not (why != "").any(), _summary(why)
    k = np.maximum(c.self_ids, 0)
    own = (ref["id"] == c.self_ids) & ~c.ambiguous
    P0 = pairs(c.g, c.rays, k)
    tn = _f32(np.maximum(P0.lo1, 0.0011))
    pn, nn, fn = record_of(c.g, c.rays, k, tn)
    away = own & (ref["t"] > tn + 3 * tol_of(ref["t"]))
    assert away.sum() > 500, int(away.sum())
    h = ref.copy()
    h["t"][away], h["p"][away], h["normal"][away], h["front_face"][away] = tn[away], pn[away], _f32(nn[away]), fn[away]
    w, _ = check_spheres(c, h)
    assert (w[away] != "").all() and set(_summary(w[away])) <= {"t"}, _summary(w[away])


# ---- GPU ---------------------------------------------------------------------------------
def _trace(S, M, rays, oid=None, prec=N.RT_PREC_F32, T=None, **tuning):
    with N.Renderer(0, SEED, prec) as r:
        if tuning:
            r.set_tuning(**tuning)
        r.upload_scene(S, M, T)
        big = r.scene_info().big_spheres
        return r.trace_rays_host(rays if prec == N.RT_PREC_F64 else rays.astype(np.float32), oid), big


def _assert_accepted(name, c, h, only=None):
    """Every ray's record (only: of the rays marked) passes check_spheres."""
    why, ratios = check_spheres(c, h)
    if only is not None:
        why = np.where(only, why, "")
    ref = c.reference_hits()
    print(name, "same id as the exact closest hit", float((h["id"] == ref["id"]).mean()), "ambiguous",
          float(c.ambiguous.mean()), "front face uncertain", float(c.face_uncertain.mean()),
          "max error over bound", ratios, "violations", _summary(why))
    bad = np.flatnonzero(why != "")
    assert len(bad) == 0, (_summary(why), [(int(i), c.kinds[c.kind[i]], why[i], int(h["id"][i]), float(h["t"][i]),
                                            int(c.id1[i]), float(c.t1[i])) for i in bad[:8]])


GRAZING = pytest.mark.xfail(strict=True, reason="a grazing ray's roots cannot meet tol in fp32: see the test's docstring")


@pytest.mark.gpu
@pytest.mark.parametrize("name,front", [pytest.param(n, None, marks=[GRAZING] if n == "tangent" else []) for n in PLAIN] +
                         [("field", 0), ("field", 16)])
def test_trace_spheres_fp32_per_ray(name, front):
    """fp32 rt_trace_rays: every ray's record satisfies check_spheres (field: with the default
    front list, none, and 16 spheres in it; the other classes with the default).
    tangent cannot meet tol by construction and is expected to fail at it: where the margin m
    is within a few E of 0, the roots b / a -+ sqrt(2 |r| m) / |d| move by up to
    sqrt(2 |r| E) / |d| for an error E of m -- for r = 0.2 seen from 1 to 3 away, E = 2e-7 ..
    4e-7 and 3e-4 .. 4e-4 of length against tol |d| = 1e-4 .. 3e-4.  Measured on MI355X: 94 of
    8,000 rays miss tol on t (every other rule holds for all 8,000); the largest |t - root| is
    reported by test_trace_spheres_tangent_roots_conditioned, which checks the same records
    with E carried through the roots' condition."""
    sn, c = case(name)
    h, big = _trace(c.S, c.M, c.rays, **({} if front is None else {"front_spheres": front}))
    assert big == int(c.g.big.sum()), (big, int(c.g.big.sum()))
    _assert_accepted(name, c, h)


def conditioned_case(name):
    """The class `name` again as a conditioned case (Case(conditioned=True))."""
    key = name + " (conditioned)"
    if key not in _CASES:
        sn, c = case(name)
        _CASES[key] = (sn, Case(c.S, c.M, c.rays, c.self_ids, c.kind, c.kinds, conditioned=True))
    return _CASES[key]


@pytest.mark.gpu
def test_trace_spheres_tangent_roots_conditioned():
    """The tangent class again, every rule as before except that an admissible root is the
    range it takes while the margin moves by -+E (a conditioned case): what fp32 can deliver
    for grazing rays, from the same bound E."""
    sn, c = case("tangent")
    h, _ = _trace(c.S, c.M, c.rays)
    why, _ = check_spheres(c, h)
    off = np.flatnonzero(why == "t")
    k = np.clip(h["id"][off], 0, c.g.n - 1)
    P = pairs(c.g, c.rays[off], k)
    miss = np.minimum(np.abs(h["t"][off] - P.lo1), np.abs(h["t"][off] - P.lo2)) / tol_of(h["t"][off])
    print("tangent at tol:", _summary(why), "largest |t - root| / tol", float(miss.max(initial=0.0)))
    _assert_accepted("tangent (conditioned)", conditioned_case("tangent")[1], h)


def _short(c):
    return np.array(c.kinds)[c.kind] == "short"


@pytest.mark.gpu
@pytest.mark.parametrize("name", FROM)
def test_trace_spheres_from_fp32_per_ray(name):
    """fp32 rt_trace_rays_from, origins at the fp64 reference's hit points rounded to fp32: the
    Lambertian, reflected, refracted and totally reflected rays at tol (on the ground class the
    short rays too), and every ray, the short ones included, as a conditioned case."""
    sn, c = case(name)
    h, big = _trace(c.S, c.M, c.rays, c.self_ids)
    assert big == int(c.g.big.sum())
    _assert_accepted(name, c, h, only=None if name == "from_ground" else ~_short(c))
    _assert_accepted(name + " (conditioned)", conditioned_case(name)[1], h)


SHORT = pytest.mark.xfail(strict=True, reason="2 b / a of a short ray across the normal cannot meet tol in fp32: see the "
                          "test's docstring")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [pytest.param(n, marks=SHORT) for n in ("from_field", "from_HOLLOW", "from_SHELL", "short")])
def test_trace_spheres_from_short_rays_at_tol(name):
    """The short rays (|d| from 1e-6 to 1e-2, across the normal) at tol: expected to fail.  The
    origin sphere's only root is t = 2 b / a with b = -f.d, and for such a direction b is what
    cancellation leaves of |f| |d|: an error of C_B U |f| |d| in b is E_T = 2 C_B U |f| / |d|
    in t -- 2.4e-3 for r = 0.2 and |d| = 1e-4, 0.24 for |d| = 1e-6 -- against tol = 1e-4.  No
    way of writing b in fp32 avoids it short of a compensated product, which the render
    kernels do not pay for: such a root moves the ray's origin by E_T |d| = 2 C_B U |f|, a few
    ulp of the sphere.  Measured on MI355X (800 short rays a class; `short`: 8,000): field 157,
    HOLLOW 100, SHELL 104, `short` 1,574 rays break a rule at tol, nearly all of them `t` on
    the origin sphere; every one passes as a conditioned case
    (test_trace_spheres_from_fp32_per_ray, ..._device_origins_...)."""
    sn, c = case(name)
    h, _ = _trace(c.S, c.M, c.rays, c.self_ids)
    _assert_accepted(name + " (short rays at tol)", c, h, only=_short(c))


@pytest.mark.gpu
@pytest.mark.parametrize("name", FROM + ["short"])
def test_trace_spheres_from_device_origins_fp32_per_ray(name):
    """fp32 rt_trace_rays_from, origins and ids the device's own fp32 records of a first
    rt_trace_rays -- what a caller that chains the two calls gets: every kind but the short
    rays at tol, and every ray as a conditioned case."""
    sn = FROM_SCENE[name]
    S, M = scene(sn)
    with N.Renderer(0, SEED, N.RT_PREC_F32) as r:
        r.upload_scene(S, M)
        first = r.trace_rays_host(first_batch(sn).astype(np.float32))
        _, rays, oid, kind, kinds = from_case(name, first)
        assert np.array_equal(_f32(rays[:, 0:3]), rays[:, 0:3])      # fp32 records: nothing to round
        h = r.trace_rays_host(rays.astype(np.float32), oid)
    c = Case(S, M, rays, oid, kind, kinds, conditioned=True)
    assert (name == "short" or c.ambiguous.mean() <= 0.05) and c.certain_hit.mean() >= 0.25
    _assert_accepted(name + " (device origins, conditioned)", c, h)
    if name != "short":
        rest = np.flatnonzero(~_short(c))
        c = Case(S, M, rays[rest], oid[rest], kind[rest], kinds)
        _assert_accepted(name + " (device origins)", c, h[rest])


# ---- the config-5 mixed scene: origins on spheres and on triangles ------------------------
class MixedCase:
    """Rays that start on the spheres and triangles of test_trace_mesh's mixed scene.  Sphere
    candidates are judged by check_spheres, triangle candidates by test_trace_mesh.check_fp32
    with the origin triangle masked out; both against one t*, the smallest certain-hit
    distance over spheres and triangles."""

    def __init__(self, rays, oid, kind, kinds, conditioned=False):
        import test_trace_mesh as TM
        S, M, T = TM.scene("mixed")[:3]
        nS = len(S)
        self.sph = Case(S, M, rays, oid, kind, kinds, conditioned=conditioned)   # (a triangle's id is no sphere's)
        self.kind, self.kinds, self.rays, self.oid = self.sph.kind, self.sph.kinds, self.sph.rays, np.asarray(oid)
        t = TM.Case32.__new__(TM.Case32)
        t.name, t.S, t.M, t.rays, t.kind, t.kinds, t.p_floor = "from_mixed", S, M, self.rays, kind, kinds, False
        t.T = T.copy()
        for f in ("v0", "v1", "v2"):
            t.T[f] = _f32(T[f])
        t.t64, t.cmiss, t.chit, t.nd_neg, t.nd_sure = TM.fp32_classify(t.T, t.rays)
        nrm = np.cross(t.T["v1"] - t.T["v0"], t.T["v2"] - t.T["v0"])
        t.unit_n = nrm / _norm(nrm)[:, None]
        # the spheres as check_fp32 sees them: the certain closest sphere hit
        sure = np.isfinite(self.sph.tstar)
        t.sid, t.ts = np.where(sure, self.sph.id1, -1), np.where(sure, self.sph.tstar, 0.0)
        self.tri, self.nS = t, nS
        self.skip = np.where(self.oid >= nS, self.oid - nS, -1)
        masked = np.flatnonzero(self.skip >= 0)
        chit, cmiss = t.chit.copy(), t.cmiss.copy()
        chit[masked, self.skip[masked]], cmiss[masked, self.skip[masked]] = False, True
        tt = np.where(chit, t.t64, np.inf)
        both = np.minimum(tt.min(axis=1), self.sph.tstar)
        lim = np.where(np.isfinite(both), both + tol_of(both), np.inf)
        self.ambiguous = self.sph.ambiguous | (~cmiss & ~chit & (t.t64 < lim[:, None])).any(axis=1)
        lim2 = np.where(np.isfinite(both), both + 2 * tol_of(both), -np.inf)
        close = (tt <= lim2[:, None]).sum(axis=1)
        self.tied = self.sph.tied | (close >= 2) | ((close >= 1) & (self.sph.tstar <= lim2))
        self.certain_hit = np.isfinite(both) & ~self.ambiguous
        self.certain_miss = self.sph.all_miss & cmiss.all(axis=1)
        self.sph.tstar = both
        # the exact closest hit: the sphere case's, or a nearer triangle (tri_matrices' rule)
        tm = TM.tri_matrices(t.T, t.rays)[0]
        tm[masked, self.skip[masked]] = np.inf
        self.tri_k, self.tri_t = tm.argmin(axis=1), tm.min(axis=1)

    def reference_hits(self):
        import test_trace_mesh as TM
        h = self.sph.reference_hits()
        ts = np.where(self.sph.id1 >= 0, self.sph.t1, np.inf)
        w = self.tri_t < ts
        t = _f32(np.where(w, self.tri_t, 0.0))
        p, nrm, front = TM.tri_record(self.tri.T, self.rays, self.tri_k, t)
        h["t"][w], h["p"][w], h["normal"][w], h["front_face"][w] = t[w], _f32(p[w]), _f32(nrm[w]), front[w]
        h["id"][w], h["mat"][w] = self.nS + self.tri_k[w], self.tri.T["mat"][self.tri_k[w]]
        return h

    def check(self, h):
        """-> why, per ray: a sphere report by check_spheres, a triangle or a miss by check_fp32."""
        import test_trace_mesh as TM
        why_t, _ = TM.check_fp32(self.tri, h, skip=self.skip)
        on_sphere = (h["id"] >= 0) & (h["id"] < self.nS)
        hs = h.copy()
        hs[~on_sphere] = np.zeros(1, N.HIT_DTYPE)
        hs["id"][~on_sphere] = -1
        why_s, ratios = check_spheres(self.sph, hs)
        return np.where(on_sphere, why_s, why_t), ratios


def mixed_first():
    """The first batch on the mixed scene and its fp64 hit records (test_trace_mesh)."""
    import test_trace_mesh as TM
    if "mixed_first" not in _CASES:
        S, M, T, rays, _, _ = TM.class_rays("mixed")
        rays = _f32(rays)
        _CASES["mixed_first"] = (rays,) + tuple(TM.mesh_hit_reference(S, M, T, rays)[1:5])
    return _CASES["mixed_first"]


def mixed_case(conditioned=False):
    """from_mixed: 4,000 rays of every kind from the fp64 hit points of test_trace_mesh's mixed
    class, half from those on its spheres (the ground excepted), half from those on its
    triangles."""
    key = "from_mixed" + (" (conditioned)" if conditioned else "")
    if key not in _CASES:
        first, p, nrm, front, ids = mixed_first()
        nS = len(scene("field")[0])
        parts = [scattered(first, p, nrm, front, ids, keep, KINDS, NRAYS // 4, seed)
                 for keep, seed in (((ids > 0) & (ids < nS), 13), (ids >= nS, 14))]
        rays, oid, kind = (np.concatenate(x) for x in zip(*parts))
        _CASES[key] = MixedCase(rays, oid, kind, list(KINDS), conditioned)
    return _CASES[key]


def test_mixed_class_caps():
    """from_mixed, from the reference alone: the caps of test_class_caps, origins on triangles
    and on spheres each at least a quarter, and the two checkers together accept the fp64
    closest hit's records rounded to fp32 -- and reject them where the origin triangle is
    reported in place of a miss or of a hit further on."""
    c = mixed_case()
    on_tri = float((c.skip >= 0).mean())
    print("from_mixed certain hit %.4f certain miss %.4f ambiguous %.4f tied %.4f origins on triangles %.3f" %
          (c.certain_hit.mean(), c.certain_miss.mean(), c.ambiguous.mean(), c.tied.mean(), on_tri))
    assert c.ambiguous.mean() <= 0.05 and c.tied.mean() <= 0.01
    assert c.certain_hit.mean() >= 0.25 and c.certain_miss.mean() >= 0.05
    assert on_tri == 0.5
    ref = c.reference_hits()
    why, ratios = c.check(ref)
    assert not (why != "").any(), _summary(why)
    # the origin triangle itself, with its own record at a plausible t
    import test_trace_mesh as TM
    w = (c.skip >= 0) & ~c.ambiguous
    k = np.maximum(c.skip, 0)
    t = np.full(len(ref), 0.01)
    p, nrm, front = TM.tri_record(c.tri.T, c.rays, k, t)
    h = ref.copy()
    h["t"][w], h["p"][w], h["normal"][w], h["front_face"][w] = t[w], _f32(p[w]), _f32(nrm[w]), front[w]
    h["id"][w], h["mat"][w] = c.nS + k[w], c.tri.T["mat"][k[w]]
    why, _ = c.check(h)
    assert w.sum() > 500 and (why[w] != "").all(), (int((why[w] == "").sum()), int(w.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "gpu", "lbvh"])
def test_trace_mixed_from_fp32_per_ray(builder):
    """fp32 rt_trace_rays_from on the mixed scene, all three mesh builders: origins on spheres
    and on triangles (the mesh loops skip the origin triangle), every kind but the short rays
    at tol, every ray with the sphere side as a conditioned case."""
    import test_trace_mesh as TM
    c = mixed_case()
    with N.Renderer(0, SEED, N.RT_PREC_F32) as r:
        r.set_tuning(mesh_builder=TM.BUILDERS[builder])
        r.upload_scene(c.tri.S, c.tri.M, c.tri.T)
        h = r.trace_rays_host(c.rays.astype(np.float32), c.oid)
    for cc, only, label in ((c, ~_short(c), "at tol"), (mixed_case(conditioned=True), None, "conditioned")):
        why, ratios = cc.check(h)
        if only is not None:
            why = np.where(only, why, "")
        print("from_mixed", builder, label, "same id as the exact closest hit", float((h["id"] == cc.reference_hits()["id"]).mean()),
              "ambiguous", float(cc.ambiguous.mean()), "max error over bound (spheres)", ratios, "violations", _summary(why))
        bad = np.flatnonzero(why != "")
        assert len(bad) == 0, (label, _summary(why), [(int(i), cc.kinds[cc.kind[i]], why[i], int(h["id"][i]), float(h["t"][i]),
                                                       int(cc.oid[i])) for i in bad[:8]])


def _same_records(a, b):
    return all(np.array_equal(a[f], b[f]) for f in ("t", "p", "normal", "id", "front_face", "mat"))


def _trace_from_null(r, rays):
    """rt_trace_rays_from with origin_ids = NULL."""
    import torch
    rays = np.ascontiguousarray(rays, dtype=r.dtype).reshape(-1, 7)
    d_rays = torch.from_numpy(rays).to("cuda")
    d_hits = torch.empty(len(rays) * N.HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.trace_rays_from(d_rays.data_ptr(), len(rays), 0, d_hits.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_hits.cpu().numpy().view(N.HIT_DTYPE)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["field", "mixed_host", "mixed_gpu", "mixed_lbvh"])
def test_trace_rays_from_without_ids_is_trace_rays(where):
    """fp32: rt_trace_rays_from with NULL, with all -1 and with ids outside the scene's range
    returns rt_trace_rays' records bit for bit, on the field and on the mixed scene with all
    three mesh builders."""
    import test_trace_mesh as TM
    if where == "field":
        S, M = field()
        T, rays, tuning = None, _rays(4000, seed=21), {}
    else:
        S, M, T, rays, _, _ = TM.class_rays("mixed")
        tuning = {"mesh_builder": TM.BUILDERS[where[len("mixed_"):]]}
    n = len(rays)
    total = len(S) + (0 if T is None else len(T))
    outside = np.array([-1, -2, total, total + 1, np.iinfo(np.int32).min, np.iinfo(np.int32).max])[np.arange(n) % 6]
    with N.Renderer(0, SEED, N.RT_PREC_F32) as r:
        if tuning:
            r.set_tuning(**tuning)
        r.upload_scene(S, M, T)
        base = r.trace_rays_host(rays.astype(np.float32))
        assert (base["id"] >= 0).mean() > 0.3
        assert _same_records(base, _trace_from_null(r, rays))
        assert _same_records(base, r.trace_rays_host(rays.astype(np.float32), np.full(n, -1)))
        assert _same_records(base, r.trace_rays_host(rays.astype(np.float32), outside))


@pytest.mark.gpu
def test_trace_rays_from_fp64_ignores_the_ids():
    """fp64: rt_trace_rays_from with real origin ids equals rt_trace_rays bit for bit and still
    equals world_hit_reference (the reference has no self rule)."""
    sn, c = case("short")
    rays = c.rays
    t, p, nrm, ff, ids = world_hit_reference(c.S, c.M, rays)
    with N.Renderer(0, SEED, N.RT_PREC_F64) as r:
        r.upload_scene(c.S, c.M)
        base = r.trace_rays_host(rays)
        got = r.trace_rays_host(rays, c.self_ids)
    assert _same_records(base, got)
    hit = ids >= 0
    assert (ids == c.self_ids).mean() >= 0.03           # the reference does re-hit the origin sphere
    assert np.array_equal(got["id"], ids) and np.array_equal(got["t"][hit], t[hit])
    assert np.array_equal(got["p"][hit], p[hit]) and np.array_equal(got["normal"][hit], nrm[hit])
    assert np.array_equal(got["front_face"][hit].astype(bool), ff[hit])
    assert np.array_equal(got["mat"][hit], c.S["mat"][ids[hit]])
