// Fused passes of the Laplace approximation of binary Gaussian process
// classification (gpc.py; the host side is _laplace.py; Rasmussen & Williams,
// algorithms 3.1 and 5.1 with the logistic link).  All matrices are row-major
// float64 n x n and symmetric; y holds 0 / 1.  One Newton step is
//
//   lp_build -> potrf.hip (B^-1, log|L_B|) -> lp_solve -> lp_apply
//
// and the lp_build of the next step also sums the objective of this one, so a
// step costs three launches of this file.
//
// lp_build: one wave per row i of K.  From the latent values f it forms
// pi = sigmoid(f), w = pi (1 - pi), s = sqrt(w), g = y - pi, b = w f + g
// (every wave for every column j: n^2 exponentials instead of one more
// launch), writes B[i, j] = delta_ij + (s_i K_ij) s_j and
// vec = [pi, s, b, g, K b] (5 n).  Wave 0 of workgroup 0 also sums, for the f
// and a it was given (the result of the step before),
// sums = [a . f, sum_j log1p(exp(-(2 y_j - 1) f_j))].
// lp_solve: one wave per row of B^-1: a_i = b_i - s_i sum_j B^-1_ij s_j (K b)_j.
// lp_apply: one wave per row of K: f_i = sum_j K_ij a_j.
// lp_planes_*: the gradient of the objective as ONE contraction of the
// kernel's gradient planes with M = (a a^T - s B^-1 s + u g^T + g u^T) / 2,
// formed on the fly from B^-1 and vecs = [s, a, u, g] (4 n).  The planes are
// read in the type the solver stored them in, float or double, at
// P[i s_lane + j s_col + pidx[k] s_k]; the host picks the lane axis with the
// smaller stride (the planes are symmetric).  A workgroup of four waves takes
// one 64 x 16 block of a 64 x 64 tile (I, J), I <= J: a lane per row, a wave
// per column at a time, KC planes per chunk in registers; column i of row j
// of B^-1 is contiguous along the lanes.  Tiles off the diagonal count twice.
// Each workgroup reduces its KC sums (wave shuffles, then the four waves in
// order) into partial[k * nblk + block].
// lp_reduce: dense_reduce.h's reduce_partials, one workgroup per plane.
// The grids are functions of the shapes alone and there are no atomics: the
// same bits on every call.
#include "dense_reduce.h"

#define TILE 64
#define SUB 4                    // column blocks per tile (TILE / SUB columns)

__device__ __forceinline__ double sigmoid(double x) {
    if (x >= 0.0) return 1.0 / (1.0 + exp(-x));
    const double e = exp(x);
    return e / (1.0 + e);
}

// gridDim.x = ceil(n / NWAVE)
extern "C" __global__ __launch_bounds__(BLOCK) void
lp_build(const double *__restrict__ K, int64_t n, const double *__restrict__ f,
         const double *__restrict__ y, const double *__restrict__ a,
         double *__restrict__ B, double *__restrict__ vec,
         double *__restrict__ sums)
{
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t i = (int64_t)blockIdx.x * NWAVE + wid;
    if (i >= n) return;                       // (whole waves only)
    const bool summing = blockIdx.x == 0 && wid == 0;     // (wave-uniform)
    const double fi = f[i];
    const double pi = sigmoid(fi), wi = pi * (1.0 - pi), si = sqrt(wi);
    const double *ki = K + i * n;
    double *bi = B + i * n;
    double kb = 0.0, sa = 0.0, sl = 0.0;
    for (int64_t j = lane; j < n; j += WAVE) {
        const double fj = f[j], yj = y[j];
        const double pj = sigmoid(fj), wj = pj * (1.0 - pj);
        const double kij = ki[j];
        kb += kij * (wj * fj + (yj - pj));
        bi[j] = (i == j ? 1.0 : 0.0) + (si * kij) * sqrt(wj);
        if (summing) {
            sa += a[j] * fj;
            sl += log1p(exp(-(2.0 * yj - 1.0) * fj));
        }
    }
    kb = wave_sum(kb);
    if (summing) {
        sa = wave_sum(sa);
        sl = wave_sum(sl);
    }
    if (lane == 0) {
        const double gi = y[i] - pi;
        vec[i] = pi;
        vec[n + i] = si;
        vec[2 * n + i] = wi * fi + gi;
        vec[3 * n + i] = gi;
        vec[4 * n + i] = kb;
        if (summing) {
            sums[0] = sa;
            sums[1] = sl;
        }
    }
}

// vec as lp_build wrote it; gridDim.x = ceil(n / NWAVE)
extern "C" __global__ __launch_bounds__(BLOCK) void
lp_solve(const double *__restrict__ Binv, int64_t n,
         const double *__restrict__ vec, double *__restrict__ a)
{
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t i = (int64_t)blockIdx.x * NWAVE + wid;
    if (i >= n) return;
    const double *s = vec + n, *kb = vec + 4 * n, *ri = Binv + i * n;
    double t = 0.0;
    for (int64_t j = lane; j < n; j += WAVE) t += ri[j] * (s[j] * kb[j]);
    t = wave_sum(t);
    if (lane == 0) a[i] = vec[2 * n + i] - s[i] * t;
}

// gridDim.x = ceil(n / NWAVE)
extern "C" __global__ __launch_bounds__(BLOCK) void
lp_apply(const double *__restrict__ K, int64_t n, const double *__restrict__ a,
         double *__restrict__ f)
{
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t i = (int64_t)blockIdx.x * NWAVE + wid;
    if (i >= n) return;
    const double *ki = K + i * n;
    double t = 0.0;
    for (int64_t j = lane; j < n; j += WAVE) t += ki[j] * a[j];
    t = wave_sum(t);
    if (lane == 0) f[i] = t;
}

template <typename T, int KC>
__device__ __forceinline__ void planes_stage(
    const T *__restrict__ P, int64_t n, int64_t s_lane, int64_t s_col,
    int64_t s_k, const int64_t *__restrict__ pidx, int nt,
    const double *__restrict__ Binv, const double *__restrict__ vecs,
    int64_t ntiles, double *__restrict__ partial)
{
    const int64_t blk = blockIdx.x % (ntiles * SUB);
    const int64_t t = blk / SUB;
    const int sub = (int)(blk % SUB);
    const int k0 = (int)(blockIdx.x / (ntiles * SUB)) * KC;
    const int nk = min(KC, nt - k0);
    // tile t -> (I, J), I <= J, column by column: t = J (J + 1) / 2 + I
    int64_t J = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (J * (J + 1) / 2 > t) --J;
    while ((J + 1) * (J + 2) / 2 <= t) ++J;
    const int64_t I = t - J * (J + 1) / 2;

    __shared__ double red[NWAVE][KC];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t i = I * TILE + lane;
    const double *s = vecs, *a = vecs + n, *u = vecs + 2 * n, *g = vecs + 3 * n;
    int64_t off[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk)
        off[kk] = kk < nk ? pidx[k0 + kk] * s_k : 0;
    double acc[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) acc[kk] = 0.0;
    if (i < n) {
        const double si = s[i], ai = a[i], ui = u[i], gi = g[i];
        const T *pi = P + i * s_lane;
        const int64_t c0 = J * TILE + sub * (TILE / SUB);
        const int64_t c1 = min(c0 + TILE / SUB, n);
        for (int64_t j = c0 + wid; j < c1; j += NWAVE) {
            const double w = 0.5 * ((ai * a[j] - (si * Binv[j * n + i]) * s[j])
                                    + (ui * g[j] + gi * u[j]));
            const T *pj = pi + j * s_col;
#pragma unroll
            for (int kk = 0; kk < KC; ++kk)
                if (kk < nk) acc[kk] += w * (double)pj[off[kk]];
        }
    }
    const double weight = I == J ? 1.0 : 2.0;
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) {
        const double r = wave_sum(acc[kk]);
        if (lane == 0) red[wid][kk] = r;
    }
    __syncthreads();
    if (threadIdx.x < nk) {
        double r = 0.0;
        for (int w = 0; w < NWAVE; ++w) r += red[w][threadIdx.x];
        partial[(int64_t)(k0 + threadIdx.x) * (ntiles * SUB) + blk] =
            weight * r;
    }
}

#define PLANES(T, SFX, KC)                                                     \
    extern "C" __global__ __launch_bounds__(BLOCK) void                        \
    lp_planes_##SFX##_k##KC(const T *P, int64_t n, int64_t s_lane,             \
                            int64_t s_col, int64_t s_k, const int64_t *pidx,   \
                            int nt, const double *Binv, const double *vecs,    \
                            int64_t ntiles, double *partial) {                 \
        planes_stage<T, KC>(P, n, s_lane, s_col, s_k, pidx, nt, Binv, vecs,    \
                            ntiles, partial);                                  \
    }

PLANES(float, f32, 1)
PLANES(float, f32, 2)
PLANES(float, f32, 4)
PLANES(float, f32, 8)
PLANES(float, f32, 16)
PLANES(double, f64, 1)
PLANES(double, f64, 2)
PLANES(double, f64, 4)
PLANES(double, f64, 8)
PLANES(double, f64, 16)

// gridDim.x = nt: out[k] = sum of the nblk partials of plane k, fixed order
extern "C" __global__ __launch_bounds__(BLOCK) void
lp_reduce(const double *__restrict__ partial, int64_t nblk,
          double *__restrict__ out)
{
    reduce_partials(partial, nblk, out);
}
