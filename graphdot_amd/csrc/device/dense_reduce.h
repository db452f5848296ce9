// Workgroup shape and reductions shared by the fused dense kernels (the .hip
// files next to the models that use them; DESIGN.md, "Fused dense kernels"):
// 256 threads = four wave64, double sums in a fixed order, no atomics.
//
// There are two wave sums in this tree and they are NOT interchangeable: they
// add the 64 lanes in different orders and so differ in the last bits.
//   wave_sum (here): the __shfl_xor butterfly; every lane gets the total.
//     Used by lowrank.hip, field.hip, outlier.hip, select.hip, laplace.hip,
//     subspace.hip and lloyd.hip.
//   graphdot::wave::sum (wave.h): DPP row sums chained into lane 63.  Used by
//     posterior.hip and the solvers.
// A kernel that moved from one to the other would change its results.
#ifndef GRAPHDOT_HIP_DENSE_REDUCE_H_
#define GRAPHDOT_HIP_DENSE_REDUCE_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BLOCK 256
#define WAVE 64
#define NWAVE (BLOCK / WAVE)

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
