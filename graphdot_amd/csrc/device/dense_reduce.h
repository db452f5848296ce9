// Workgroup shape, reductions and small helpers shared by the fused dense
// kernels (the .hip files next to the models that use them; DESIGN.md, "Fused
// dense kernels"): 256 threads = four wave64, double sums in a fixed order, no
// atomics.
//
// There are two wave sums in this tree and they are NOT interchangeable: they
// add the 64 lanes in different orders and so differ in the last bits.
//   wave_sum (here): the __shfl_xor butterfly; every lane gets the total.
//     Used by lowrank.hip, field.hip, outlier.hip, select.hip, laplace.hip,
//     subspace.hip, lloyd.hip, alignment.hip and mmd.hip.
//   graphdot::wave::sum (wave.h): DPP row sums chained into lane 63.  Used by
//     posterior.hip and the solvers.
// A kernel that moved from one to the other would change its results.
// (smo.hip and svr.hip use neither: their butterflies pick a working set, they
// add nothing.  They take BLOCK, WAVE, NWAVE and is_finite from here.
// potrf.hip does not include this header.)
#ifndef GRAPHDOT_HIP_DENSE_REDUCE_H_
#define GRAPHDOT_HIP_DENSE_REDUCE_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BLOCK 256
#define WAVE 64
#define NWAVE (BLOCK / WAVE)

// (smo.hip, svr.hip, lloyd.hip)
__device__ __forceinline__ bool is_finite(double x) {
    return fabs(x) < __builtin_inf();
}

// VEC consecutive elements of a matrix row as doubles, in one load: p is
// 16-byte aligned where VEC > 1 (lloyd.hip, subspace.hip)
template <typename T, int VEC>
__device__ __forceinline__ void load_k(const T *p, double (&out)[VEC]) {
    if constexpr (VEC == 1) {
        out[0] = (double)p[0];
    } else if constexpr (sizeof(T) == 4) {
        const float4 v = *reinterpret_cast<const float4 *>(p);
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    } else {
        const double2 v = *reinterpret_cast<const double2 *>(p);
        out[0] = v.x; out[1] = v.y;
    }
}

// One SMO step's update of the pair (i, j) along the constraint, clipped to
// its box (libsvm's two cases; the last clamp guards the partner, a rounded
// difference): declares `ni` and `nj`, the new alpha_i and alpha_j.  DIFFER:
// the two variables have opposite signs.  A macro, because as an inline
// function (reference outputs, or a pair returned by value) it changed the
// instruction streams of svm_smo_* and svm_smo2_* (smo.hip, svr.hip).
#define SMO_PAIR_UPDATE(DIFFER, a_i, a_j, G_i, G_j, U_i, U_j, q)               \
    double ni, nj;                                                             \
    if (DIFFER) {                                                              \
        const double delta = (-G_i - G_j) / q, diff = a_i - a_j;               \
        ni = a_i + delta;                                                      \
        nj = a_j + delta;                                                      \
        if (diff > 0.0) {                                                      \
            if (nj < 0.0) { nj = 0.0; ni = diff; }                             \
        } else {                                                               \
            if (ni < 0.0) { ni = 0.0; nj = -diff; }                            \
        }                                                                      \
        if (diff > U_i - U_j) {                                                \
            if (ni > U_i) { ni = U_i; nj = U_i - diff; }                       \
        } else {                                                               \
            if (nj > U_j) { nj = U_j; ni = U_j + diff; }                       \
        }                                                                      \
    } else {                                                                   \
        const double delta = (G_i - G_j) / q, sum = a_i + a_j;                 \
        ni = a_i - delta;                                                      \
        nj = a_j + delta;                                                      \
        if (sum > U_i) {                                                       \
            if (ni > U_i) { ni = U_i; nj = sum - U_i; }                        \
        } else {                                                               \
            if (nj < 0.0) { nj = 0.0; ni = sum; }                              \
        }                                                                      \
        if (sum > U_j) {                                                       \
            if (nj > U_j) { nj = U_j; ni = sum - U_j; }                        \
        } else {                                                               \
            if (ni < 0.0) { ni = 0.0; nj = sum; }                              \
        }                                                                      \
    }                                                                          \
    ni = ni < 0.0 ? 0.0 : (ni > U_i ? U_i : ni);                               \
    nj = nj < 0.0 ? 0.0 : (nj > U_j ? U_j : nj)

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

// NaN-propagating maximum (a NaN among the inputs must reach the output)
__device__ __forceinline__ double nanmax(double a, double b) {
    return (a != a || a > b) ? a : b;
}

__device__ __forceinline__ double wave_max(double v) {
    for (int off = WAVE / 2; off > 0; off >>= 1)
        v = nanmax(v, __shfl_xor(v, off, WAVE));
    return v;
}

// Stage 2 of a two-stage sum: out[j] = sum_b partial[j nblk + b] for workgroup
// j = blockIdx.x, b in a fixed order (strided over the threads, the butterfly,
// then the four waves in order): the same bits on every call.
__device__ __forceinline__ void reduce_partials(
    const double *__restrict__ partial, int64_t nblk, double *__restrict__ out)
{
    __shared__ double red[NWAVE];
    const double *p = partial + (int64_t)blockIdx.x * nblk;
    double s = 0.0;
    for (int64_t b = threadIdx.x; b < nblk; b += BLOCK) s += p[b];
    s = wave_sum(s);
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    if (lane == 0) red[wid] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < NWAVE; ++w) t += red[w];
        out[blockIdx.x] = t;
    }
}

#endif
