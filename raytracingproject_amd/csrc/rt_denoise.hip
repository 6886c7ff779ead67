// rt_denoise.hip -- the translation unit of rt_denoise's kernels (rt_denoise.h), both precisions.
// Built with -ffp-contract=off and nothing that relaxes fp32: division and square root are
// correctly rounded and denormals are kept, so the device follows the rule of include/rt_hip.h
// bit for bit.  (rt_render_f32.hip's flags flush denormals and relax fp32 divide / sqrt.)
#include "rt_denoise.h"

#include "rt_launch.h"

namespace rtx {

namespace {

template <class T>
hipError_t denoise_launches(const DenoiseLaunch& D, hipStream_t stream) {
    using V4 = typename DnVec<T>::type;
    const size_t npix = (size_t)D.width * (size_t)D.height;
    DenoiseArgs<T> A;
    A.W = D.width, A.H = D.height;
    A.samples = D.samples, A.guide_samples = D.guide_samples;
    A.sums = (const T*)D.sums, A.sumsq = (const T*)D.sumsq, A.counts = D.counts;
    A.albedo = (const T*)D.albedo, A.hits = D.hits, A.normal = (const T*)D.normal, A.depth = (const T*)D.depth;
    V4 *a = (V4*)D.col_a, *b = (V4*)D.col_b, *g = (V4*)D.guide;
    const dim3 flat((unsigned)((npix + 255) / 256)), block(256);
    hipLaunchKernelGGL(denoise_prepare_kernel<T>, flat, block, 0, stream, A, a, g);
    if (!D.sumsq) hipLaunchKernelGGL(denoise_spatial_variance_kernel<T>, flat, block, 0, stream, D.width, D.height, (T*)a);
    // (64-bit: width and height go up to 2^31 - 1)
    const int tiles_x = (int)(((long long)D.width + DN_BLOCK_X - 1) / DN_BLOCK_X);
    const int tiles_y = (int)(((long long)D.height + DN_BLOCK_Y - 1) / DN_BLOCK_Y);
    const dim3 tiles((unsigned)((size_t)tiles_x * (size_t)tiles_y));
    for (int i = 0; i < D.iterations; ++i) {
        hipLaunchKernelGGL(denoise_atrous_kernel<T>, tiles, dim3(DN_BLOCK_X * DN_BLOCK_Y), 0, stream, D.width, D.height,
                           tiles_x, 1 << i, D.normal_log2_power, (T)D.sigma_depth, (T)D.sigma_lum, (T)D.lum_eps,
                           (const V4*)a, (const V4*)g, b);
        V4* t = a;
        a = b, b = t;
    }
    hipLaunchKernelGGL(denoise_finish_kernel<T>, flat, block, 0, stream, A, (const V4*)a, (T*)D.out,
                       (T*)D.out_variance);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_denoise(const DenoiseLaunch& D, hipStream_t stream) {
    return D.elem_bytes == 8 ? denoise_launches<double>(D, stream) : denoise_launches<float>(D, stream);
}

}  // namespace rtx
