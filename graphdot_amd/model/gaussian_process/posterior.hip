// Fused posterior of a Gaussian process for a handful of candidates
// (_device_posterior.py; the host side is _posterior.py).  Given the inverse
// Kinv (n x n, float64, row-major) of the regularised training matrix, the
// cross kernel Ks of b candidates against the n training samples, column-major
// as the solver leaves it (element (c, j) at Ks[c + j b], float or double),
// Ky = Kinv y, the regularised prior diagonal kss (b) and the scaling of the
// targets, it produces
//
//   t[r, c] = sum_j Kinv[r, j] Ks[c, j]
//   mean[c] = ystd * sum_r Ks[c, r] Ky[r] + ymean
//   std[c]  = ystd * sqrt(max(0, kss[c] - sum_r Ks[c, r] t[r, c]))
//
// in out[2 b] = [mean | std], and on request T (n x b, row-major) = t.
//
// gp_rows_* (stage A): a wave per row r of Kinv, four rows per workgroup, KC
// candidates per register chunk (the chunk is the slow grid axis:
// blockIdx.x = chunk * nblk + row block).  The lanes stride over j two
// columns at a time (one 16-byte load of Kinv per lane and step where the row
// is 16-byte aligned, i.e. n even); the KC values of a column j are contiguous
// in Ks.  Everything is accumulated in double.  After the wave sums lane kk
// holds t[r, c0 + kk]: it stores it into T, multiplies by Ks[c, r] and the four
// waves are summed in order into partial[c * nblk + blk] (the quadratic form)
// and partial[(b + c) * nblk + blk] (the mean).  Kinv -- the only large
// operand -- is read once per chunk of 16 candidates.
// gp_finish (stage B): workgroup c sums its two rows of partials in a fixed
// order and applies the epilogue.  The grids and the order of every sum are
// functions of (n, b) alone and there are no atomics: the same bits on every
// call.
#include "dense_reduce.h"
#include "wave.h"

template <typename T, int KC>
__device__ __forceinline__ void rows_stage(
    const double *__restrict__ Kinv, const T *__restrict__ Ks,
    const double *__restrict__ Ky, int64_t n, int b, int64_t nblk,
    double *__restrict__ partial, double *__restrict__ Tout)
{
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t blk = blockIdx.x % nblk;
    const int c0 = (int)(blockIdx.x / nblk) * KC;
    const int nk = min(KC, b - c0);
    const int64_t r = blk * NWAVE + wid;
    const bool live = r < n;                  // (whole waves only)

    double acc[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) acc[kk] = 0.0;
    if (live) {
        const double *kr = Kinv + r * n;
        const T *ks = Ks + c0;
        const int64_t npair = n / 2;
        if ((n & 1) == 0) {
            const double2 *kr2 = reinterpret_cast<const double2 *>(kr);
            for (int64_t p = lane; p < npair; p += WAVE) {
                const double2 v = kr2[p];
                const T *k0 = ks + 2 * p * b, *k1 = k0 + b;
#pragma unroll
                for (int kk = 0; kk < KC; ++kk)
                    if (kk < nk) {
                        acc[kk] += v.x * (double)k0[kk];
                        acc[kk] += v.y * (double)k1[kk];
                    }
            }
        } else {
            for (int64_t p = lane; p < npair; p += WAVE) {
                const double vx = kr[2 * p], vy = kr[2 * p + 1];
                const T *k0 = ks + 2 * p * b, *k1 = k0 + b;
#pragma unroll
                for (int kk = 0; kk < KC; ++kk)
                    if (kk < nk) {
                        acc[kk] += vx * (double)k0[kk];
                        acc[kk] += vy * (double)k1[kk];
                    }
            }
            if (lane == 0) {                  // the odd last column
                const double v = kr[n - 1];
                const T *k0 = ks + (n - 1) * b;
#pragma unroll
                for (int kk = 0; kk < KC; ++kk)
                    if (kk < nk) acc[kk] += v * (double)k0[kk];
            }
        }
    }
    // lane kk keeps the sum of candidate c0 + kk
    double mine = 0.0;
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) {
        const double s = graphdot::wave::sum(acc[kk]);
        if (lane == kk) mine = s;
    }
    __shared__ double red[NWAVE][2][KC];
    if (lane < KC) {
        double q = 0.0, m = 0.0;
        if (live && lane < nk) {
            const double k = (double)Ks[c0 + lane + r * b];
            q = k * mine;
            m = k * Ky[r];
            if (Tout) Tout[r * b + c0 + lane] = mine;
        }
        red[wid][0][lane] = q;
        red[wid][1][lane] = m;
    }
    __syncthreads();
    if ((int)threadIdx.x < nk) {
        double q = 0.0, m = 0.0;
        for (int w = 0; w < NWAVE; ++w) {
            q += red[w][0][threadIdx.x];
            m += red[w][1][threadIdx.x];
        }
        const int64_t c = c0 + threadIdx.x;
        partial[c * nblk + blk] = q;
        partial[(b + c) * nblk + blk] = m;
    }
}

#define ROWS(T, SFX, KC)                                                       \
    extern "C" __global__ __launch_bounds__(BLOCK) void                        \
    gp_rows_##SFX##_k##KC(const double *Kinv, const T *Ks, const double *Ky,   \
                          int64_t n, int b, int64_t nblk, double *partial,     \
                          double *Tout) {                                      \
        rows_stage<T, KC>(Kinv, Ks, Ky, n, b, nblk, partial, Tout);            \
    }

ROWS(float, f32, 1)
ROWS(float, f32, 2)
ROWS(float, f32, 4)
ROWS(float, f32, 8)
ROWS(float, f32, 16)
ROWS(double, f64, 1)
ROWS(double, f64, 2)
ROWS(double, f64, 4)
ROWS(double, f64, 8)
ROWS(double, f64, 16)

__device__ __forceinline__ double block_sum(const double *__restrict__ src,
                                            int64_t len, double *red)
{
    double s = 0.0;
    for (int64_t q = threadIdx.x; q < len; q += BLOCK) s += src[q];
    s = graphdot::wave::sum(s);
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    __syncthreads();                          // (red is used twice)
    if (lane == 0) red[wid] = s;
    __syncthreads();
    double t = red[0];
    for (int w = 1; w < NWAVE; ++w) t += red[w];
    return t;
}

// gridDim.x = b; out = [mean (b) | std (b)]
extern "C" __global__ __launch_bounds__(BLOCK) void
gp_finish(const double *__restrict__ partial, int64_t nblk, int b,
          const double *__restrict__ kss, double ymean, double ystd,
          double *__restrict__ out)
{
    __shared__ double red[NWAVE];
    const int64_t c = blockIdx.x;
    const double q = block_sum(partial + c * nblk, nblk, red);
    const double m = block_sum(partial + (b + c) * nblk, nblk, red);
    if (threadIdx.x == 0) {
        out[c] = ystd * m + ymean;
        const double v = kss[c] - q;          // (a NaN stays one)
        out[b + c] = ystd * sqrt(v < 0.0 ? 0.0 : v);
    }
}
