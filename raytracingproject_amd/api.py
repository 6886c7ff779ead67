"""Python mirror of the reference's header API (src/camera.h, hittable_list.h, bvh.h,
sphere.h, material.h), driving the MI355X renderer through the C ABI.

Same class names, constructor arguments and public camera fields as the reference, so
code written against the reference reads the same:

    world = hittable_list()
    world.add(sphere((0, -1000, 0), 1000, lambertian((0.5, 0.5, 0.5))))
    cam = camera()                      # the reference's CPUImpl::Camera slot
    cam.image_width = 400; ...
    cam.render(world)                   # PPM P3 on stdout, as camera.h:32-50

The C++ mirror (include/rt/*.h) is the drop-in for C++ callers; this module is what the
tests and bench use.  There is no CPU path here: render() and ray_color() run on the GPU.
"""
from __future__ import annotations

import sys
from typing import Sequence

import numpy as np

from . import _native as N
from . import rtweekend

Vec = Sequence[float]


# ---- materials (material.h:15-82) -------------------------------------------------
class material:
    type: int = -1


class lambertian(material):
    type = N.RT_LAMBERTIAN

    def __init__(self, albedo: Vec):
        self.albedo = tuple(float(x) for x in albedo)


class metal(material):
    type = N.RT_METAL

    def __init__(self, albedo: Vec, f: float):
        self.albedo = tuple(float(x) for x in albedo)
        self.fuzz = f if f < 1 else 1.0  # material.h:33


class dielectric(material):
    type = N.RT_DIELECTRIC

    def __init__(self, index_of_refraction: float):
        self.ir = float(index_of_refraction)


# ---- hittables (sphere.h, hittable_list.h, bvh.h) ------------------------------------
class hittable:
    pass


class sphere(hittable):
    """sphere(center, radius, mat) or sphere(center1, center2, radius, mat) (sphere.h:9-28)."""

    def __init__(self, *args):
        if len(args) == 3:
            center, radius, mat = args
            self.center1 = tuple(float(x) for x in center)
            self.center_vec = (0.0, 0.0, 0.0)
            self.is_moving = False
        elif len(args) == 4:
            c1, c2, radius, mat = args
            self.center1 = tuple(float(x) for x in c1)
            # center_vec = _center2 - _center1 (sphere.h:27)
            self.center_vec = tuple(float(b) - float(a) for a, b in zip(c1, c2))
            self.is_moving = True
        else:
            raise TypeError("sphere(center, radius, mat) or sphere(center1, center2, radius, mat)")
        self.radius = float(radius)
        self.mat = mat


class hittable_list(hittable):
    def __init__(self, obj: hittable | None = None):
        self.objects: list[hittable] = []
        if obj is not None:
            self.add(obj)

    def clear(self) -> None:
        self.objects.clear()

    def add(self, obj: hittable) -> None:
        self.objects.append(obj)


class bvh_node(hittable):
    """bvh_node(list) (bvh.h:10): the device layer always builds an SAH BVH over the
    list at upload, so this node simply wraps the list it was given."""

    def __init__(self, lst: hittable_list):
        self.list = lst


class triangle_mesh(hittable):
    """An indexed triangle mesh with one material (mesh path; the
    reference has no triangle primitive: its model loader is an empty stub,
    src/vulkan/model_loader.h:17-19).  vertices[nv, 3], faces[nt, 3] (0-based)."""

    def __init__(self, vertices, faces, mat: material):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        if len(self.faces) and (self.faces.min() < 0 or self.faces.max() >= len(self.vertices)):
            raise ValueError("face index out of range")
        self.mat = mat

    @classmethod
    def from_obj(cls, path, mat: material) -> "triangle_mesh":
        """Wavefront OBJ through rt_obj_load (positions + faces, fan-triangulated)."""
        V, F, _ = N.obj_load(path)
        return cls(V, F, mat)


def flatten(world: hittable) -> tuple[np.ndarray, np.ndarray]:
    """Flatten a sphere-only hittable graph into the rt_sphere / rt_material arrays of
    the C ABI (flatten_scene also returns the triangles of meshes)."""
    S, M, T = flatten_scene(world)
    if len(T):
        raise TypeError("world holds triangle meshes: use flatten_scene")
    return S, M


def flatten_scene(world: hittable) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Flatten a hittable graph into the rt_sphere / rt_material / rt_triangle arrays of
    the C ABI.  Materials shared between objects (shared_ptr in the reference) stay
    shared."""
    spheres: list[sphere] = []
    meshes: list[triangle_mesh] = []

    def walk(h: hittable) -> None:
        if isinstance(h, sphere):
            spheres.append(h)
        elif isinstance(h, triangle_mesh):
            meshes.append(h)
        elif isinstance(h, hittable_list):
            for o in h.objects:
                walk(o)
        elif isinstance(h, bvh_node):
            walk(h.list)
        else:
            raise TypeError(f"cannot flatten {type(h).__name__}")

    walk(world)
    mats: dict[int, int] = {}
    mat_objs: list[material] = []

    def mat_index(m: material) -> int:
        if id(m) not in mats:
            mats[id(m)] = len(mat_objs)
            mat_objs.append(m)
        return mats[id(m)]

    S = np.zeros(len(spheres), dtype=N.SPHERE_DTYPE)
    for k, s in enumerate(spheres):
        S[k]["center"] = s.center1
        S[k]["radius"] = s.radius
        S[k]["center_vec"] = s.center_vec
        S[k]["mat"] = mat_index(s.mat)
        S[k]["moving"] = 1 if s.is_moving else 0
    T = np.concatenate([N.triangles(m.vertices, m.faces, mat_index(m.mat)) for m in meshes]) if meshes else \
        np.zeros(0, N.TRIANGLE_DTYPE)
    M = np.zeros(len(mat_objs), dtype=N.MATERIAL_DTYPE)
    for k, m in enumerate(mat_objs):
        M[k]["type"] = m.type
        if isinstance(m, (lambertian, metal)):
            M[k]["albedo"] = m.albedo
        if isinstance(m, metal):
            M[k]["fuzz"] = m.fuzz
        if isinstance(m, dielectric):
            M[k]["ir"] = m.ir
    return S, M, T


# ---- camera (camera.h:10-126) --------------------------------------------------------
class camera:
    """Public fields of camera.h:15-26 with the same defaults."""

    def __init__(self, device: int = 0, seed: int = 0x5EED, precision: int = N.RT_PREC_F32):
        self.aspect_ratio = 1.0
        self.image_width = 100
        self.samples_per_pixel = 10
        self.max_depth = 10
        self.vfov = 90.0
        self.lookfrom = (0.0, 0.0, -1.0)
        self.lookat = (0.0, 0.0, 0.0)
        self.vup = (0.0, 1.0, 0.0)
        self.defocus_angle = 0.0
        self.focus_dist = 10.0
        self.device, self.seed, self.precision = device, seed, precision
        self._cam: N.RtCamera | None = None
        self._renderer: N.Renderer | None = None
        self._tape_renderer: N.Renderer | None = None
        self._scene_key = None

    def _desc(self) -> N.RtCameraDesc:
        d = N.RtCameraDesc()
        d.aspect_ratio = self.aspect_ratio
        d.image_width = self.image_width
        d.samples_per_pixel = self.samples_per_pixel
        d.max_depth = self.max_depth
        d.vfov = self.vfov
        d.lookfrom[:] = self.lookfrom
        d.lookat[:] = self.lookat
        d.vup[:] = self.vup
        d.defocus_angle = self.defocus_angle
        d.focus_dist = self.focus_dist
        return d

    def initialize(self) -> None:
        """camera.h:52-85 (in the library, fp64, reference operation order)."""
        self._cam = N.camera_initialize(self._desc())

    @property
    def image_height(self) -> int:
        if self._cam is None:
            self.initialize()
        return self._cam.image_height

    def image_size(self) -> tuple[int, int]:
        return self.image_width, self.image_height

    @property
    def native(self) -> N.RtCamera:
        if self._cam is None:
            self.initialize()
        return self._cam

    def _upload(self, r: N.Renderer, world: hittable) -> None:
        S, M, T = flatten_scene(world)
        r.upload_scene(S, M, T if len(T) else None)

    def render_arrays(self, world: hittable):
        """The render step without the text output: (sums, rgb, segments) on the host."""
        self.initialize()
        if self._renderer is None:
            self._renderer = N.Renderer(self.device, self.seed, self.precision)
        self._upload(self._renderer, world)
        return self._renderer.render_frame(self._cam, self.samples_per_pixel, self.max_depth)

    def render(self, world: hittable, out=None) -> None:
        """camera::render (camera.h:32-50): PPM P3 to `out` (default stdout)."""
        out = sys.stdout if out is None else out
        _, rgb, _ = self.render_arrays(world)
        write_ppm(out, rgb)

    # -- single-ray entry points of the reference API (tests.cpp:41-42) ---------------
    def get_ray(self, i: int, j: int):
        """camera.h:87-113 on the global reference stream (host, fp64)."""
        c = self.native
        du, dv = c.pixel_delta_u, c.pixel_delta_v
        pc = [(c.pixel00_loc[a] + i * du[a]) + j * dv[a] for a in range(3)]
        px = -0.5 + rtweekend.random_double()
        py = -0.5 + rtweekend.random_double()
        ps = [pc[a] + ((px * du[a]) + (py * dv[a])) for a in range(3)]
        if self.defocus_angle <= 0:
            origin = list(c.center)
        else:
            while True:  # random_in_unit_disk (vec3.h:121-127), y drawn first (g++ order)
                y = rtweekend.random_double(-1, 1)
                x = rtweekend.random_double(-1, 1)
                if x * x + y * y + 0.0 * 0.0 < 1:
                    break
            origin = [(c.center[a] + x * c.defocus_disk_u[a]) + y * c.defocus_disk_v[a] for a in range(3)]
        direction = [ps[a] - origin[a] for a in range(3)]
        time = rtweekend.random_double()
        return (*origin, *direction, time)

    def ray_color(self, r, depth: int, world: hittable):
        """camera_cpu.h:8-26 for ONE ray on the GPU (fp64), continuing the global
        reference stream: the device consumes a tape cut from a copy of the stream and
        the host stream then advances by exactly the number of uniforms used."""
        if self._tape_renderer is None:
            self._tape_renderer = N.Renderer(self.device, self.seed, N.RT_PREC_F64)
        key = id(world)
        if self._scene_key != key:
            self._upload(self._tape_renderer, world)
            self._scene_key = key
        n = 256
        while True:
            probe = rtweekend.stream().copy()
            tape = np.array([probe.canonical() for _ in range(n)], dtype=np.float64)
            col, used = self._tape_renderer.trace_tape(r, depth, tape)
            if used <= n:
                break
            n = used * 2
        for _ in range(used):
            rtweekend.random_double()
        return col

    def ray_colors(self, rays, depth: int, world: hittable, keys=None) -> np.ndarray:
        """camera_cpu.h:8-26 for MANY rays on the GPU (rt_radiance_rays), the batched counterpart
        of ray_color: rays[n, 7] (origin, direction, time) -> radiance[n, 3] in the camera's
        precision.  Ray i draws from the counter stream of keys[i] (N.RtPathKey: pixel, sample,
        first_draw; None: {i, 0, 0}) under the camera's seed; the global reference stream is not
        touched.  Runs on the camera's own renderer, as render does."""
        if self._renderer is None:
            self._renderer = N.Renderer(self.device, self.seed, self.precision)
        self._upload(self._renderer, world)
        return self._renderer.radiance_rays_host(rays, keys, depth)

    def render_pixels(self, world: hittable, pixels, sample_begin: int = 0, sample_count: int | None = None) -> np.ndarray:
        """The sums camera::render accumulates (camera.h:40-44), for chosen pixels only
        (rt_render_pixels): pixels[n, 2] of (i, j) = (column, row) -> sums[n, 3] in the camera's
        precision, over samples [sample_begin, sample_begin + sample_count) of each (default
        count: samples_per_pixel) -- the values render_arrays returns at those pixels, bit for bit.
        A pixel outside the image gives 0.  Runs on the camera's own renderer, as render does."""
        self.initialize()
        if self._renderer is None:
            self._renderer = N.Renderer(self.device, self.seed, self.precision)
        self._upload(self._renderer, world)
        ij = np.asarray(pixels, dtype=np.int64).reshape(-1, 2)
        W, H = self._cam.image_width, self._cam.image_height
        inside = (ij[:, 0] >= 0) & (ij[:, 0] < W) & (ij[:, 1] >= 0) & (ij[:, 1] < H)
        jobs = np.zeros(len(ij), N.RtPixelJob)
        jobs["pixel"] = np.where(inside, ij[:, 1] * W + ij[:, 0], 0xFFFFFFFF)
        jobs["sample_begin"] = sample_begin
        jobs["sample_count"] = self.samples_per_pixel if sample_count is None else sample_count
        return self._renderer.render_pixels_host(self._cam, jobs, self.max_depth)

    def render_adaptive(self, world: hittable, rel_error: float, abs_floor: float = 0.0, min_samples: int = 16,
                        max_samples: int | None = None, max_step: int | None = None):
        """The frame with a per-pixel sample count (Renderer.render_adaptive: rt_render_pixels_moments
        and rt_refine_jobs in rounds): every pixel takes samples 0, 1, ... of its own stream until the
        standard error of its mean is within rel_error of max(|mean|, abs_floor), between min_samples
        and max_samples (default: samples_per_pixel).  -> (mean[H, W, 3] = sums / n in the camera's
        precision, n int32[H, W]); rt_quantize(mean, spp = 1) quantises the mean."""
        self.initialize()
        if self._renderer is None:
            self._renderer = N.Renderer(self.device, self.seed, self.precision)
        self._upload(self._renderer, world)
        hi = self.samples_per_pixel if max_samples is None else max_samples
        sums, _, n, _ = self._renderer.render_adaptive(self._cam, self.max_depth, rel_error, abs_floor,
                                                       min(min_samples, hi), hi, max_step)
        sums, n = sums.cpu().numpy(), n.cpu().numpy()
        return sums / n[..., None].astype(sums.dtype), n

    def render_aov(self, world: hittable, samples: int | None = None) -> dict:
        """The guide images a denoiser asks for (rt_render_pixels_aov), from the first hits of
        samples 0 .. samples - 1 of every pixel (default: samples_per_pixel), the camera rays render
        traces: {"albedo": [H, W, 3] and "normal": [H, W, 3], the per-job sums divided by the
        sample count (misses count 0: blend with "coverage" for a sky colour); "depth": [H, W], the
        nearest hit's ray parameter (times focus_dist: planar depth; +inf for sky); "id": int32[H, W],
        its primitive in the upload's order (-1 for sky); "coverage": [H, W], hits / samples}."""
        self.initialize()
        if self._renderer is None:
            self._renderer = N.Renderer(self.device, self.seed, self.precision)
        self._upload(self._renderer, world)
        n = self.samples_per_pixel if samples is None else samples
        W, H = self._cam.image_width, self._cam.image_height
        jobs = np.zeros(W * H, N.RtPixelJob)
        jobs["pixel"], jobs["sample_count"] = np.arange(W * H), n
        o = self._renderer.render_pixels_aov_host(self._cam, jobs)
        dt = o["albedo"].dtype.type
        return {"albedo": (o["albedo"] / dt(n)).reshape(H, W, 3), "normal": (o["normal"] / dt(n)).reshape(H, W, 3),
                "depth": o["depth"].reshape(H, W), "id": o["id"].reshape(H, W),
                "coverage": (o["hits"].astype(o["albedo"].dtype) / dt(n)).reshape(H, W)}

    def render_denoised(self, world: hittable, samples: int | None = None, counts=None, **params) -> dict:
        """The frame at `samples` per pixel (default: samples_per_pixel), denoised on the device
        (rt_denoise): a full-frame job list through rt_render_pixels_moments and
        rt_render_pixels_aov, then the a-trous filter guided by albedo, normal, depth and the
        samples' own variance.  params: rt_denoise_params' fields (iterations, normal_log2_power,
        sigma_depth, sigma_lum, lum_eps); the rest keep the library's defaults.
        counts: Renderer.render_adaptive's (sums, sumsq, n) -- device tensors or arrays -- in place
        of the uniform render: the filter divides by the per-pixel n, and the guides still come
        from samples 0 .. samples - 1.
        -> {"color": [H, W, 3] the denoised mean, "noisy": [H, W, 3] sums / n, "variance": [H, W]
        the filtered variance of the demodulated channel average}, in the camera's precision."""
        self.initialize()
        if self._renderer is None:
            self._renderer = N.Renderer(self.device, self.seed, self.precision)
        r = self._renderer
        self._upload(r, world)
        spp = self.samples_per_pixel if samples is None else samples
        W, H = self._cam.image_width, self._cam.image_height
        jobs = np.zeros(W * H, N.RtPixelJob)
        jobs["pixel"], jobs["sample_count"] = np.arange(W * H), spp
        g = r.render_pixels_aov_host(self._cam, jobs)
        if counts is None:
            sums, sumsq = r.render_pixels_moments_host(self._cam, jobs, self.max_depth)
            n = None
        else:
            sums, sumsq, n = (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a) for a in counts)
            sums, sumsq = sums.reshape(-1, 3).astype(r.dtype), sumsq.reshape(-1, 3).astype(r.dtype)
            n = n.reshape(-1).astype(np.uint32)
        out, var = r.denoise_host(W, H, sums, sumsq, n, spp if n is None else 0, g["albedo"], g["normal"], g["depth"],
                                  g["hits"], spp, N.Renderer.denoise_params(**params))
        with np.errstate(divide="ignore", invalid="ignore"):
            noisy = sums / r.dtype(spp) if n is None else np.where(n[:, None] > 0, sums / n[:, None].astype(r.dtype), 0)
        return {"color": out.reshape(H, W, 3), "noisy": noisy.astype(r.dtype).reshape(H, W, 3),
                "variance": var.reshape(H, W)}


def write_ppm(out, rgb: np.ndarray) -> None:
    """PPM P3 exactly as camera.h:35 and color.h:32-34 print it."""
    H, W, _ = rgb.shape
    out.write(f"P3\n{W} {H}\n255\n")
    flat = rgb.reshape(-1, 3)
    out.write("".join(f"{r} {g} {b}\n" for r, g, b in flat.tolist()))
