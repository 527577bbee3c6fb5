// tsp_perspective.hip -- perspective camera (tsp_project_perspective, include/topsy_splat.h "Perspective view").
//
// No splat kernel of its own: to first order across a footprint, a perspective view of SPH particles is the orthographic view of
// a transformed snapshot.  A particle at distance d along the optical axis is seen as if it lay on the reference plane at
// distance D: position scaled by s = D / d, smoothing length h s, mass m s^2 -- so m' / h'^2, the vertex weight, is unchanged
// and with it the column density along the ray through the particle's centre.  One streaming kernel writes that snapshot into a
// second context, with the vertex weights (weights_kernel, tsp_data.hip) and the bounds of every BOUNDS_BLOCK particles
// (block_bounds_kernel) in the same pass; kernels S / N / H2 then draw it as they draw any other.
// Arithmetic in the order written, no contraction (-ffp-contract=off), so that a numpy restatement gives the same bits.
#include <cmath>

#include "tsp_internal.h"

namespace tsp {

struct PerspectiveArgs {
    const float *x, *y, *z, *h, *m, *r, *g, *b;            // src (m, r, g, b: nullptr when not resident)
    float *ox, *oy, *oz, *oh, *om, *orr, *og, *ob, *wm;    // dst
    float4 *bounds;
    int64_t n;
    tsp_perspective cam;
};

constexpr int PER_LANE = BOUNDS_BLOCK / 64;     // particles of a block per lane

// HBM-bound: 20 B in and 24 B out per particle (12 + 12 more with rgb), 32 B per block.  One wave per block of BOUNDS_BLOCK
// particles, four blocks per workgroup (the waves share nothing: no LDS, no barrier); lane l takes particles l, 64 + l, ...: every
// load and store instruction of the wave covers 256 consecutive bytes, and the 8 loads of an array are independent, so a lane has
// 32 (56 with rgb) dwords in flight before the first use.  The bounds are reduced across the wave by __shfl_xor.
__global__ __launch_bounds__(256) void perspective_kernel(const PerspectiveArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t i0 = blk * BOUNDS_BLOCK;
    if (i0 >= a.n) return;                                   // (the whole wave)
    const bool mass = a.m != nullptr, rgb = a.r != nullptr;
    float X[PER_LANE], Y[PER_LANE], Z[PER_LANE], H[PER_LANE], M[PER_LANE], R[PER_LANE], G[PER_LANE], B[PER_LANE];
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
        const int64_t i = i0 + k * 64 + lane;
        const bool in = i < a.n;
        X[k] = in ? a.x[i] : 0.0f;
        Y[k] = in ? a.y[i] : 0.0f;
        Z[k] = in ? a.z[i] : 0.0f;
        H[k] = in ? a.h[i] : 0.0f;
        M[k] = in && mass ? a.m[i] : 0.0f;
        R[k] = in && rgb ? a.r[i] : 0.0f;
        G[k] = in && rgb ? a.g[i] : 0.0f;
        B[k] = in && rgb ? a.b[i] : 0.0f;
    }
    const float *rot = a.cam.rot, *off = a.cam.offset;
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf}, hm = -inf;
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
        const int64_t i = i0 + k * 64 + lane;
        if (i >= a.n) continue;
        const float tx = X[k] + off[0], ty = Y[k] + off[1], tz = Z[k] + off[2];
        const float xv = (rot[0] * tx + rot[1] * ty) + rot[2] * tz;
        const float yv = (rot[3] * tx + rot[4] * ty) + rot[5] * tz;
        const float zv = (rot[6] * tx + rot[7] * ty) + rot[8] * tz;
        const float d = a.cam.distance - zv;                  // the viewer sits at zv = +distance and looks down -z
        const bool visible = d >= a.cam.near;                 // (false for NaN)
        const float s = a.cam.distance / d, ss = s * s;
        const float v[3] = {visible ? xv * s : nan, visible ? yv * s : nan, visible ? zv : nan};
        const float hp = visible ? H[k] * s : 0.0f;
        a.ox[i] = v[0];
        a.oy[i] = v[1];
        a.oz[i] = v[2];
        a.oh[i] = hp;
        if (mass) {
            const float mp = visible ? M[k] * ss : 0.0f;
            a.om[i] = mp;
            const float hh = hp * hp;                          // weights_kernel's expression (tsp_data.hip)
            a.wm[i] = mp / hh;
        }
        if (rgb) {
            a.orr[i] = visible ? R[k] * ss : 0.0f;
            a.og[i] = visible ? G[k] * ss : 0.0f;
            a.ob[i] = visible ? B[k] * ss : 0.0f;
        }
        // block_bounds_kernel's rules: fminf / fmaxf drop NaN operands
        for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], v[c]); hi[c] = fmaxf(hi[c], v[c]); }
        hm = fmaxf(hm, hp);
    }
    for (int o = 32; o; o >>= 1) {
        for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o)); }
        hm = fmaxf(hm, __shfl_xor(hm, o));
    }
    if (lane == 0) {
        a.bounds[2 * blk] = make_float4(lo[0], lo[1], lo[2], hm);
        a.bounds[2 * blk + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

}  // namespace tsp

using namespace tsp;

extern "C" int tsp_project_perspective(tsp_context *src, tsp_context *dst, const tsp_perspective *cam) {
    TSP_REQUIRE(src && dst && cam, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(src != dst, TSP_EINVAL, "src and dst must be two contexts");
    TSP_REQUIRE(src->device == dst->device, TSP_EINVAL, "src is on device %d, dst on device %d", src->device, dst->device);
    TSP_REQUIRE(std::isfinite(cam->distance) && cam->distance > 0.0f, TSP_EINVAL, "distance must be finite and > 0, not %.9g", (double)cam->distance);
    TSP_REQUIRE(std::isfinite(cam->near) && cam->near > 0.0f && cam->near < cam->distance, TSP_EINVAL,
                "near must be finite, > 0 and < distance, not %.9g", (double)cam->near);
    for (int k = 0; k < 9; ++k) TSP_REQUIRE(std::isfinite(cam->rot[k]), TSP_EINVAL, "rot must be finite");
    for (int k = 0; k < 3; ++k) TSP_REQUIRE(std::isfinite(cam->offset[k]), TSP_EINVAL, "offset must be finite");
    const Particles &s = src->p;
    Particles &d = dst->p;
    TSP_REQUIRE(s.n > 0 && s.x && s.y && s.z && s.h, TSP_ESTATE, "src holds no particles");
    TSP_REQUIRE(d.n > 0 && d.x && d.y && d.z && d.h, TSP_ESTATE, "dst holds no particles: upload the snapshot into it once");
    TSP_REQUIRE(s.n == d.n, TSP_EINVAL, "src holds %lld particles, dst %lld", (long long)s.n, (long long)d.n);
    TSP_REQUIRE((s.m != nullptr) == (d.m != nullptr), TSP_ESTATE, "the mass array is resident in %s only", s.m ? "src" : "dst");
    const bool s_rgb = s.r && s.g && s.b, d_rgb = d.r && d.g && d.b;
    TSP_REQUIRE(s_rgb == d_rgb, TSP_ESTATE, "the rgb arrays are resident in %s only", s_rgb ? "src" : "dst");
    TSP_HIP(hipSetDevice(dst->device));
    // the only allocations, under the sites of the calls that own them; nothing of dst has changed when one of them fails
    int rc;
    if (d.m && !d.wm && (rc = ensure_weights(dst, false))) return rc;
    const int64_t blocks = (d.n + BOUNDS_BLOCK - 1) / BOUNDS_BLOCK;
    if (!dst->ws.bounds_valid && (!dst->ws.block_bounds || dst->ws.bounds_capacity < blocks) && (rc = ensure_block_bounds(dst))) return rc;
    if ((rc = check_workspace(dst))) return rc;
    TSP_REQUIRE(dst->ws.block_bounds && dst->ws.bounds_capacity >= blocks && (!d.m || d.wm), TSP_ESTATE, "dst's weights or block bounds are missing");

    PerspectiveArgs a;
    a.x = s.x; a.y = s.y; a.z = s.z; a.h = s.h; a.m = s.m;
    a.r = s_rgb ? s.r : nullptr; a.g = s_rgb ? s.g : nullptr; a.b = s_rgb ? s.b : nullptr;
    a.ox = d.x; a.oy = d.y; a.oz = d.z; a.oh = d.h; a.om = d.m; a.orr = d.r; a.og = d.g; a.ob = d.b; a.wm = d.wm;
    a.bounds = dst->ws.block_bounds;
    a.n = d.n;
    a.cam = *cam;
    // what src's stream still has to write (an upload, a reorder) comes first
    TSP_HIP(hipEventRecord(src->ev[EV_T0], src->stream));
    TSP_HIP(hipStreamWaitEvent(dst->stream, src->ev[EV_T0], 0));
    // from here on dst changes
    d.wm_valid = false;
    d.wrgb_source = W_NONE;                                    // (the rgb weights are re-formed by the next rgb block)
    dst->ws.bounds_valid = false;
    dst->cell_offsets.clear();                                 // (the cell grid described world coordinates; the strata are index ranges and stay)
    dst->cell_bits = 0;
    dst->forget_render_undo();
    hipLaunchKernelGGL(perspective_kernel, dim3((unsigned)((blocks + 3) / 4)), dim3(256), 0, dst->stream, a);
    TSP_HIP(hipGetLastError());
    TSP_HIP(hipStreamSynchronize(dst->stream));               // (src may change again as soon as the call returns)
    d.wm_valid = d.m != nullptr;
    dst->ws.bounds_valid = true;
    return TSP_OK;
}
