// Fused epilogue of the outlier detector's likelihood (outlier_detector.py;
// the host side is _outlier.py).  Given the inverse Kinv of
// K_sigma = K + diag(sigma^2), the targets y and the kernel's gradient planes
// dK, it produces in one packed float64 buffer
//
//   out = [y^T a, ||K_sigma||_inf, ||Kinv||_inf, d_theta (nt), d_alpha (n)]
//
// with a = Kinv y, d_theta[k] = sum_ij (Kinv_ij - a_i a_j) dK[i, j, pidx[k]]
// and d_alpha[i] = (Kinv_ii - a_i^2) 2 sigma_i^2.  Three launches:
//
// od_rows (stage A): one wave per row of Kinv and K_sigma (both row-major
// float64 n x n); writes a_i, a_i y_i, d_alpha_i and the two absolute row
// sums into rows[5 n].
// od_planes_* (stage B): one pass over the planes on and above the diagonal.
// The planes are read in the type the solver stored them in, float or
// double, at P[i s_lane + j s_col + pidx[k] s_k]; the host picks the lane
// axis with the smaller stride (the planes are symmetric).  A workgroup of
// four waves takes one 64 x 16 block of a 64 x 64 tile (I, J), I <= J: a lane
// per row, a wave per column at a time, KC planes per chunk in registers.
// W_ij = Kinv_ji - a_i a_j is formed on the fly (Kinv is symmetric; column i
// of row j is contiguous along the lanes).  Tiles off the diagonal count
// twice.  Each workgroup reduces its KC sums (wave shuffles, then the four
// waves in order) into partial[k * nblk + block].
// od_reduce (stage C): one workgroup per scalar sums its inputs in a fixed
// order; the others copy d_alpha into place.  The grids are functions of the
// shapes alone and there are no atomics: the same bits on every call.
#include "dense_reduce.h"

#define TILE 64
#define SUB 4                    // column blocks per tile (TILE / SUB columns)

// rows: [a (n), a * y (n), d_alpha (n), |K_sigma| row sums (n), |Kinv| row
// sums (n)]; gridDim.x = ceil(n / NWAVE)
extern "C" __global__ __launch_bounds__(BLOCK) void
od_rows(const double *__restrict__ Kinv, const double *__restrict__ Ks,
        int64_t n, const double *__restrict__ y,
        const double *__restrict__ sigma2, double *__restrict__ rows)
{
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t i = (int64_t)blockIdx.x * NWAVE + wid;
    if (i >= n) return;                       // (whole waves only)
    const double *ki = Kinv + i * n, *si = Ks + i * n;
    double a = 0.0, rk = 0.0, rkinv = 0.0;
    for (int64_t j = lane; j < n; j += WAVE) {
        const double v = ki[j];
        a += v * y[j];
        rkinv += fabs(v);
        rk += fabs(si[j]);
    }
    a = wave_sum(a);
    rk = wave_sum(rk);
    rkinv = wave_sum(rkinv);
    if (lane == 0) {
        rows[i] = a;
        rows[n + i] = a * y[i];
        rows[2 * n + i] = (ki[i] - a * a) * 2.0 * sigma2[i];
        rows[3 * n + i] = rk;
        rows[4 * n + i] = rkinv;
    }
}

template <typename T, int KC>
__device__ __forceinline__ void planes_stage(
    const T *__restrict__ P, int64_t n, int64_t s_lane, int64_t s_col,
    int64_t s_k, const int64_t *__restrict__ pidx, int nt,
    const double *__restrict__ Kinv, const double *__restrict__ a,
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
    int64_t off[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk)
        off[kk] = kk < nk ? pidx[k0 + kk] * s_k : 0;
    double acc[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) acc[kk] = 0.0;
    if (i < n) {
        const double ai = a[i];
        const T *pi = P + i * s_lane;
        const int64_t c0 = J * TILE + sub * (TILE / SUB);
        const int64_t c1 = min(c0 + TILE / SUB, n);
        for (int64_t j = c0 + wid; j < c1; j += NWAVE) {
            const double w = Kinv[j * n + i] - ai * a[j];
            const T *pj = pi + j * s_col;
#pragma unroll
            for (int kk = 0; kk < KC; ++kk)
                if (kk < nk) acc[kk] += w * (double)pj[off[kk]];
        }
    }
    const double weight = I == J ? 1.0 : 2.0;
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) {
        const double s = wave_sum(acc[kk]);
        if (lane == 0) red[wid][kk] = s;
    }
    __syncthreads();
    if (threadIdx.x < nk) {
        double s = 0.0;
        for (int w = 0; w < NWAVE; ++w) s += red[w][threadIdx.x];
        partial[(int64_t)(k0 + threadIdx.x) * (ntiles * SUB) + blk] =
            weight * s;
    }
}

#define PLANES(T, SFX, KC)                                                     \
    extern "C" __global__ __launch_bounds__(BLOCK) void                        \
    od_planes_##SFX##_k##KC(const T *P, int64_t n, int64_t s_lane,             \
                            int64_t s_col, int64_t s_k, const int64_t *pidx,   \
                            int nt, const double *Kinv, const double *a,       \
                            int64_t ntiles, double *partial) {                 \
        planes_stage<T, KC>(P, n, s_lane, s_col, s_k, pidx, nt, Kinv, a,       \
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

// gridDim.x = 3 + nt + ceil(n / BLOCK).  Workgroup 0: y^T a; 1, 2: the two
// infinity norms; 3 + k: d_theta[k] from its nblk partials; the rest copy
// d_alpha into out[3 + nt + i].
extern "C" __global__ __launch_bounds__(BLOCK) void
od_reduce(const double *__restrict__ rows, int64_t n,
          const double *__restrict__ partial, int64_t nblk, int nt,
          double *__restrict__ out)
{
    const int64_t b = blockIdx.x;
    if (b >= 3 + nt) {
        const int64_t i = (b - 3 - nt) * BLOCK + threadIdx.x;
        if (i < n) out[3 + nt + i] = rows[2 * n + i];
        return;
    }
    const bool is_max = b == 1 || b == 2;
    const double *src = b == 0 ? rows + n
                      : b == 1 ? rows + 3 * n
                      : b == 2 ? rows + 4 * n
                      : partial + (b - 3) * nblk;
    const int64_t len = b < 3 ? n : nblk;
    double s = 0.0;
    for (int64_t q = threadIdx.x; q < len; q += BLOCK)
        s = is_max ? nanmax(s, src[q]) : s + src[q];
    s = is_max ? wave_max(s) : wave_sum(s);
    __shared__ double red[NWAVE];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    if (lane == 0) red[wid] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0];
        for (int w = 1; w < NWAVE; ++w)
            t = is_max ? nanmax(t, red[w]) : t + red[w];
        out[b] = t;
    }
}
