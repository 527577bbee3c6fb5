// tsp_kinematics.hip -- line-of-sight velocity maps (TSP_MODE_KINEMATIC, include/topsy_splat.h "Kinematic maps").
//
// No splat kernel of its own: the rgb kernels accumulate three weighted sums and a fragment count per pixel, so with the
// "colours" (m, m u, m u^2) of a particle, u its velocity along the line of sight, one pass leaves S = sum k m / h^2,
// A = sum k m u / h^2, B = sum k m u^2 / h^2.  Here are the two kernels around that pass:
//   * the per-particle weights, once per change of the line of sight (ensure_weights, tsp_data.hip): a pure stream, 20 B read
//     (h, m, vx, vy, vz) and 12 B written (wr, wg, wb) per particle;
//   * the per-pixel moments of a kinematic image: mean = A / S, sigma = sqrt(B / S - mean^2), in float64.
// Arithmetic in the order written, no contraction (-ffp-contract=off), so that a numpy restatement gives the same bits.
#include <algorithm>

#include "tsp_internal.h"

namespace tsp {

struct LineOfSight {
    float a[3], v[3];     // unit axis, reference velocity
};

__device__ __forceinline__ void kinematic_weight(const LineOfSight &los, float h, float m, float vx, float vy, float vz, float &wr,
                                                 float &wg, float &wb) {
    const float u = ((los.a[0] * (vx - los.v[0]) + los.a[1] * (vy - los.v[1])) + los.a[2] * (vz - los.v[2]));
    float r = m, g = m * u, b = g * u;
    if (!(finite_f32(m) && finite_f32(u))) r = g = b = 0.0f;     // such a particle draws nothing (its fragments still count)
    const float hh = h * h;                                      // weights_kernel's expression (tsp_data.hip)
    wr = r / hh; wg = g / hh; wb = b / hh;
}

// one 16-byte non-temporal load (the inputs are streamed once per pass; as a whole-vector builtin it also stays one instruction)
__device__ __forceinline__ float4 stream_load4(const float *p, int64_t i) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 t = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(p) + i);
    return make_float4(t.x, t.y, t.z, t.w);
}

// HBM-bound: grid-stride over groups of four particles, one 16-byte load per input array and one 16-byte store per output array
// and lane (every array is a device allocation of its own, so each is aligned far beyond 16 bytes), five independent loads in
// flight per lane; the n mod 4 last particles go one per lane.
__global__ __launch_bounds__(256) void kinematic_weights_kernel(const float *__restrict__ h, const float *__restrict__ m,
                                                                const float *__restrict__ vx, const float *__restrict__ vy,
                                                                const float *__restrict__ vz, int64_t n, LineOfSight los,
                                                                float *__restrict__ wr, float *__restrict__ wg, float *__restrict__ wb) {
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t i = t0; i < n4; i += stride) {
        const float4 H = stream_load4(h, i), M = stream_load4(m, i), X = stream_load4(vx, i), Y = stream_load4(vy, i), Z = stream_load4(vz, i);
        float4 R, G, B;
        kinematic_weight(los, H.x, M.x, X.x, Y.x, Z.x, R.x, G.x, B.x);
        kinematic_weight(los, H.y, M.y, X.y, Y.y, Z.y, R.y, G.y, B.y);
        kinematic_weight(los, H.z, M.z, X.z, Y.z, Z.z, R.z, G.z, B.z);
        kinematic_weight(los, H.w, M.w, X.w, Y.w, Z.w, R.w, G.w, B.w);
        reinterpret_cast<float4 *>(wr)[i] = R;
        reinterpret_cast<float4 *>(wg)[i] = G;
        reinterpret_cast<float4 *>(wb)[i] = B;
    }
    const int64_t i = (n4 << 2) + t0;
    if (i < n) kinematic_weight(los, h[i], m[i], vx[i], vy[i], vz[i], wr[i], wg[i], wb[i]);
}

int launch_kinematic_weights(tsp_context *ctx) {
    const Particles &p = ctx->p;
    TSP_REQUIRE(p.h && p.m && p.vx && p.vy && p.vz && p.wr && p.wg && p.wb, TSP_ESTATE, "kinematic weights: an array is not resident");
    LineOfSight los;
    for (int k = 0; k < 3; ++k) { los.a[k] = ctx->los[k]; los.v[k] = ctx->los[3 + k]; }
    const int64_t groups = std::max<int64_t>((p.n >> 2), 1);
    const unsigned grid = (unsigned)std::min<int64_t>((groups + 255) / 256, (int64_t)ctx->cu_count * 8);
    hipLaunchKernelGGL(kinematic_weights_kernel, dim3(grid), dim3(256), 0, ctx->stream, p.h, p.m, p.vx, p.vy, p.vz, p.n, los, p.wr, p.wg,
                       p.wb);
    TSP_HIP(hipGetLastError());
    return TSP_OK;
}

// (S, A, B, n) -> (S, mean, sigma, n) per pixel; every operation a correctly rounded IEEE one (velocity_moments_f32, tsp_math.h)
__global__ __launch_bounds__(256) void velocity_moments_kernel(const float4 *__restrict__ img, int64_t npix, float4 *__restrict__ maps) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (int64_t)gridDim.x * 256) {
        const float4 c = img[p];
        float mean, sigma;
        velocity_moments_f32(c.x, c.y, c.z, mean, sigma);
        maps[p] = make_float4(c.x, mean, sigma, c.w);
    }
}

int launch_velocity_moments(tsp_context *ctx, const float *d_img, int64_t npix, float *d_maps) {
    const unsigned grid = (unsigned)std::max<int64_t>(std::min<int64_t>((npix + 255) / 256, (int64_t)ctx->cu_count * 8), 1);
    hipLaunchKernelGGL(velocity_moments_kernel, dim3(grid), dim3(256), 0, ctx->stream, reinterpret_cast<const float4 *>(d_img), npix,
                       reinterpret_cast<float4 *>(d_maps));
    TSP_HIP(hipGetLastError());
    return TSP_OK;
}

}  // namespace tsp
