// tsp_blocks.h -- what the sphere passes over caller-ordered host arrays share (tsp_center.hip, tsp_orient.hip): blocks of CBLK
// consecutive particles, one float4 per lane and array of a 256-lane workgroup, each with the float32 bounding box of its valid
// members, and the test that lets a pass skip a block unread.
#pragma once
#include <chrono>

#include "tsp_internal.h"

namespace tsp {

constexpr int CBLK = 1024;      // particles per block: one float4 per lane of a 256-lane workgroup

__device__ __forceinline__ bool finite_position_and_mass(float x, float y, float z, float m) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z) && __builtin_isfinite(m) && m > 0.0f;
}

__device__ __forceinline__ void box_empty(float box[6]) {
    box[0] = box[1] = box[2] = __builtin_inff();
    box[3] = box[4] = box[5] = -__builtin_inff();
}

__device__ __forceinline__ void box_include(float box[6], float x, float y, float z) {
    box[0] = fminf(box[0], x);
    box[1] = fminf(box[1], y);
    box[2] = fminf(box[2], z);
    box[3] = fmaxf(box[3], x);
    box[4] = fmaxf(box[4], y);
    box[5] = fmaxf(box[5], z);
}

// the union of the lanes' boxes over the 256-lane workgroup, stored as out[0..5] = (min x, y, z, max x, y, z); every lane of the
// workgroup calls it (two barriers)
__device__ __forceinline__ void workgroup_box_store(float box[6], float *__restrict__ out) {
    __shared__ float wave_box[4][6];
    for (int off = 32; off; off >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            box[c] = fminf(box[c], __shfl_xor(box[c], off));
            box[3 + c] = fmaxf(box[3 + c], __shfl_xor(box[3 + c], off));
        }
    }
    if ((threadIdx.x & 63) == 0)
        for (int c = 0; c < 6; ++c) wave_box[threadIdx.x >> 6][c] = box[c];
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        float v = wave_box[0][c];
        for (int w = 1; w < 4; ++w) v = c < 3 ? fminf(v, wave_box[w][c]) : fmaxf(v, wave_box[w][c]);
        out[c] = v;
    }
    __syncthreads();
}

// the distance along one axis from c to the interval [lo, hi], with the subtraction d2 uses
__device__ __forceinline__ double axis_distance(float lo, float hi, double c) {
    return fmax(fmax((double)lo - c, c - (double)hi), 0.0);
}

// no point of the box has d2 < r2, d2 = (dx * dx + dy * dy) + dz * dz with dx = (double)x - cx (dy, dz alike): the box distance is
// formed with the operations and the order of d2 itself, and subtraction, squaring and addition round monotonically.  An empty
// box (+inf .. -inf) is outside every sphere.
__device__ __forceinline__ bool box_outside_sphere(const float *__restrict__ box, double cx, double cy, double cz, double r2) {
    const double gx = axis_distance(box[0], box[3], cx);
    const double gy = axis_distance(box[1], box[4], cy);
    const double gz = axis_distance(box[2], box[5], cz);
    return (gx * gx + gy * gy) + gz * gz >= r2;
}

inline double wall_ms(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace tsp
