// host_queries.cpp -- the reference's scene interface used directly, as code written
// against src/hittable.h / src/material.h would use it:
//   * a user subclass of hittable overriding hit() (a sphere that counts its tests) and
//     one with no device form (a disk: hit() and bounding_box() only);
//   * world.hit(ray, interval, rec) and rec.mat->scatter(...) called by hand, in the
//     reference's own recursion (camera_cpu.h:8-26), on the host in fp64 -- against
//     HIPImpl::Camera::ray_color, the same ray traced by the device's fp64 kernel on the
//     same global random stream: colours and stream positions must agree bit for bit;
//   * rendering a world that holds the disk is refused (std::invalid_argument);
//   * the batched form of ray_color, rt_radiance_rays, on a handful of the caller's own rays;
//   * a crop window rendered through rt_render_pixels, against the same pixels of rt_render_frame.
// Exit status 0 = pass.
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "bvh.h"
#include "camera_hip.h"
#include "hittable_list.h"
#include "material.h"
#include "sphere.h"

class counted_sphere : public sphere {
  public:
    using sphere::sphere;
    mutable long tests = 0;
    bool hit(const ray& r, interval ray_t, hit_record& rec) const override {
        ++tests;
        return sphere::hit(r, ray_t, rec);
    }
};

// A flat disk: a reference-style hittable with no flatten() (no device form).
class disk : public hittable {
  public:
    disk(point3 c, double rad, shared_ptr<material> m) : c_(c), r_(rad), m_(m) {}
    bool hit(const ray& r, interval ray_t, hit_record& rec) const override {
        const double dy = r.direction().y();
        if (dy == 0) return false;
        const double t = (c_.y() - r.origin().y()) / dy;
        if (!ray_t.surrounds(t)) return false;
        const point3 p = r.at(t);
        if ((p - c_).length_squared() > r_ * r_) return false;
        rec.t = t;
        rec.p = p;
        rec.set_face_normal(r, vec3(0, 1, 0));
        rec.mat = m_;
        return true;
    }
    aabb bounding_box() const override { return aabb(c_ - vec3(r_, 0, r_), c_ + vec3(r_, 0, r_)); }

  private:
    point3 c_;
    double r_;
    shared_ptr<material> m_;
};

// camera_cpu.h:8-26 through the virtual interface
static color host_ray_color(const ray& r, int depth, const hittable& world) {
    if (depth <= 0) return color(0, 0, 0);
    hit_record rec;
    if (world.hit(r, interval(0.001, infinity), rec)) {
        ray scattered;
        color attenuation;
        if (rec.mat->scatter(r, rec, attenuation, scattered))
            return attenuation * host_ray_color(scattered, depth - 1, world);
        return color(0, 0, 0);
    }
    const vec3 u = unit_vector(r.direction());
    const double a = 0.5 * (u.y() + 1.0);
    return (1.0 - a) * color(1.0, 1.0, 1.0) + a * color(0.5, 0.7, 1.0);
}

int main() {
    hittable_list spheres;
    spheres.add(make_shared<sphere>(point3(0, -1000, 0), 1000, make_shared<lambertian>(color(0.5, 0.5, 0.5))));
    auto counted = make_shared<counted_sphere>(point3(0, 1, 0), 1.0, make_shared<dielectric>(1.5));
    spheres.add(counted);
    spheres.add(make_shared<sphere>(point3(-4, 1, 0), 1.0, make_shared<lambertian>(color(0.4, 0.2, 0.1))));
    spheres.add(make_shared<sphere>(point3(4, 1, 0), 1.0, make_shared<metal>(color(0.7, 0.6, 0.5), 0.0)));
    for (int a = -5; a < 5; ++a)
        for (int b = -5; b < 5; ++b) {
            const double pick = random_double();
            const point3 c(a + 0.9 * random_double(), 0.2, b + 0.9 * random_double());
            if (pick < 0.6) {
                const point3 c2 = c + vec3(0, random_double(0, 0.5), 0);
                spheres.add(make_shared<sphere>(c, c2, 0.2, make_shared<lambertian>(color::random() * color::random())));
            } else if (pick < 0.85) {
                spheres.add(make_shared<sphere>(c, 0.2, make_shared<metal>(color::random(0.5, 1), random_double(0, 0.5))));
            } else {
                spheres.add(make_shared<sphere>(c, 0.2, make_shared<dielectric>(1.5)));
            }
        }
    hittable_list world;
    world.add(make_shared<bvh_node>(spheres));   // bvh_node::hit on the host: same closest hits

    HIPImpl::Camera cam;
    cam.precision = RT_PREC_F64;
    cam.aspect_ratio = 16.0 / 9.0;
    cam.image_width = 64;
    cam.vfov = 20;
    cam.lookfrom = point3(13, 2, 3);
    cam.lookat = point3(0, 0, 0);
    cam.vup = vec3(0, 1, 0);
    cam.defocus_angle = 0.6;
    cam.focus_dist = 10.0;
    cam.initialize();

    int bad = 0, rays = 0;
    long hits = 0;
    for (int j = 0; j < 36; j += 3)
        for (int i = 0; i < 64; i += 3) {
            const ray r = cam.get_ray(i, j);
            const std::mt19937 before = rt_host::generator();
            hit_record rec;
            hits += world.hit(r, interval(0.001, infinity), rec) ? 1 : 0;
            const color h = host_ray_color(r, 50, world);
            const std::mt19937 after_host = rt_host::generator();
            rt_host::generator() = before;
            const color d = cam.ray_color(r, 50, world);
            const bool same = h.x() == d.x() && h.y() == d.y() && h.z() == d.z() && rt_host::generator() == after_host;
            if (!same && bad++ < 5)
                std::printf("ray (%d,%d): host %.17g %.17g %.17g device %.17g %.17g %.17g\n", i, j, h.x(), h.y(), h.z(),
                            d.x(), d.y(), d.z());
            ++rays;
        }

    hittable_list with_disk = world;
    with_disk.add(make_shared<disk>(point3(0, 2.5, 0), 1.0, make_shared<lambertian>(color(0.9, 0.1, 0.1))));
    hit_record rec;
    const bool disk_hit = with_disk.hit(ray(point3(0, 5, 0), vec3(0, -1, 0)), interval(0.001, infinity), rec) &&
                          rec.t == 2.5 && rec.front_face;
    bool refused = false;
    try {
        cam.render(with_disk);
    } catch (const std::invalid_argument&) {
        refused = true;
    }
    // rt_radiance_rays: ray_color for a batch of the caller's own rays, each on its own counter
    // stream (pixel, sample) -- here five rays of an orthographic view looking down -z, which
    // rt_camera cannot produce.  The buffers are rt_host_alloc memory, which the device reads
    // and writes in place; rt_last_kernel_ms waits for the call.
    bool batch_ok = false, crop_ok = false;
    {
        constexpr int NR = 5;
        rt_ctx* q = rt_create(0, 0x5EED, RT_PREC_F64);
        scene_builder sb;
        world.flatten(sb);
        int rc = q ? rt_upload_scene_ex(q, sb.spheres.data(), (int)sb.spheres.size(), sb.materials.data(),
                                        (int)sb.materials.size(), sb.triangles.data(), (int)sb.triangles.size())
                   : RT_ERR_HIP;
        double* qrays = (double*)rt_host_alloc(NR * 7 * sizeof(double));
        rt_path_key* qkeys = (rt_path_key*)rt_host_alloc(NR * sizeof(rt_path_key));
        double* qrad = (double*)rt_host_alloc(NR * 3 * sizeof(double));
        uint32_t* qseg = (uint32_t*)rt_host_alloc(NR * sizeof(uint32_t));
        if (rc == RT_OK && qrays && qkeys && qrad && qseg) {
            for (int k = 0; k < NR; ++k) {
                const double ray7[7] = {-4.0 + 2.0 * k, 1.0, 8.0, 0.0, 0.0, -1.0, 0.5};
                for (int a = 0; a < 7; ++a) qrays[k * 7 + a] = ray7[a];
                qkeys[k] = rt_path_key{(uint32_t)k, 0u, 0u, 0u};
            }
            float ms = 0.f;
            rc = rt_radiance_rays(q, qrays, NR, qkeys, 50, qrad, qseg, nullptr);
            if (rc == RT_OK) rc = rt_last_kernel_ms(q, &ms);
            batch_ok = rc == RT_OK;
            for (int k = 0; k < NR && batch_ok; ++k) {
                std::printf("radiance ray %d: %.17g %.17g %.17g (%u segments)\n", k, qrad[k * 3], qrad[k * 3 + 1],
                            qrad[k * 3 + 2], qseg[k]);
                for (int a = 0; a < 3; ++a) batch_ok = batch_ok && qrad[k * 3 + a] >= 0.0 && qrad[k * 3 + a] <= 1.0;
                batch_ok = batch_ok && qseg[k] >= 1 && qseg[k] <= 50;
            }
        }
        if (rc != RT_OK) std::printf("rt_radiance_rays: %s (%s)\n", rt_error_string(rc), q ? rt_last_error(q) : "no context");
        // rt_render_pixels: a 16 x 8 crop window of the 64 x 36 frame at 4 samples per pixel, one
        // job {pixel, first sample, count} per pixel -- the sums rt_render_frame gives those pixels,
        // bit for bit, without rendering the other 2,176.
        if (rc == RT_OK) {
            constexpr int W = 64, SPP = 4, X0 = 24, Y0 = 14, CW = 16, CH = 8, NJ = CW * CH;
            rt_camera_desc desc{};
            desc.aspect_ratio = 16.0 / 9.0;
            desc.image_width = W;
            desc.vfov = 20;
            const double from[3] = {13, 2, 3}, up[3] = {0, 1, 0};
            for (int a = 0; a < 3; ++a) desc.lookfrom[a] = from[a], desc.lookat[a] = 0, desc.vup[a] = up[a];
            desc.defocus_angle = 0.6;
            desc.focus_dist = 10.0;
            rt_camera view;
            rc = rt_camera_initialize(&desc, &view);
            rt_pixel_job* jobs = (rt_pixel_job*)rt_host_alloc(NJ * sizeof(rt_pixel_job));
            double* crop = (double*)rt_host_alloc(NJ * 3 * sizeof(double));
            std::vector<double> frame(rc == RT_OK ? (size_t)W * view.image_height * 3 : 0);
            if (rc == RT_OK && jobs && crop) {
                for (int k = 0; k < NJ; ++k)
                    jobs[k] = rt_pixel_job{(uint32_t)((Y0 + k / CW) * W + X0 + k % CW), 0u, (uint32_t)SPP, 0u};
                float ms = 0.f;
                rc = rt_render_pixels(q, &view, jobs, NJ, 50, 0, crop, nullptr, nullptr);
                if (rc == RT_OK) rc = rt_last_kernel_ms(q, &ms);   // (waits for the call)
                if (rc == RT_OK) rc = rt_render_frame(q, &view, SPP, 50, frame.data(), nullptr, nullptr);
                crop_ok = rc == RT_OK;
                for (int k = 0; k < NJ && crop_ok; ++k)
                    for (int a = 0; a < 3; ++a)
                        crop_ok = crop_ok && crop[k * 3 + a] == frame[(size_t)jobs[k].pixel * 3 + a];
                std::printf("crop window %dx%d at (%d,%d): %s rt_render_frame, first pixel %.17g %.17g %.17g\n", CW, CH, X0,
                            Y0, crop_ok ? "equals" : "DIFFERS FROM", crop[0], crop[1], crop[2]);
            }
            if (rc != RT_OK) std::printf("rt_render_pixels: %s (%s)\n", rt_error_string(rc), rt_last_error(q));
            rt_host_free(jobs);
            rt_host_free(crop);
        }
        rt_host_free(qrays);
        rt_host_free(qkeys);
        rt_host_free(qrad);
        rt_host_free(qseg);
        if (q) rt_destroy(q);
    }
    const bool ok = bad == 0 && counted->tests > 0 && hits > 0 && disk_hit && refused && batch_ok && crop_ok;
    std::printf("rays %d mismatched %d world.hit %ld counted_sphere tests %ld disk_hit %d render_refused %d "
                "radiance_batch %d crop_window %d %s\n",
                rays, bad, hits, counted->tests, disk_hit, refused, batch_ok, crop_ok, ok ? "PASS" : "FAIL");
    return ok ? 0 : 1;
}
