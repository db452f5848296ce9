// Centred kernel-target alignment and its gradient as one fused pass over the
// kernel matrix and the kernel's gradient planes (kta.py; the host side is
// _align.py; Cortes, Mohri, Rostamizadeh 2012).  With
// H = I - 11^T / n, Tc = H T the centred (n, kt) targets, w_ij = Tc_i . Tc_j
// and K_c = H K H, i.e.
//
//   K_c[i, j] = K[i, j] - r_i / n - r_j / n + s / n^2,   r = K 1, s = 1^T r,
//
// the launches sum
//
//   a = sum_ij K_c[i, j] w_ij           b = sum_ij K_c[i, j]^2
//   g_p = sum_ij dK_p[i, j] w_ij        h_p = sum_ij dK_p[i, j] K_c[i, j]
//
// (the planes enter uncentred: H is a projector).  Neither K_c nor w is ever
// stored.  K and the planes are symmetric and are read in the type the solver
// stored them in, float or double, as they lie: K at K[i k_lane + j k_col],
// the planes at P[i s_lane + j s_col + pidx[p] s_k]; the host picks for each
// the lane axis with the smaller stride.  Every accumulator is double.
//
// ka_rows_*: one wave per index i, r_i = sum_l K[l k_lane + i k_col] (lanes
// strided over l, then the butterfly).
// ka_planes_*_k{KC}: one workgroup of four waves per 64 x 64 tile (I, J),
// I <= J, and chunk of KC planes: a lane per row, a wave per column at a time.
// The workgroup first sums s from r (every workgroup in the same order: the
// same bits), and puts the rows of Tc of the tile's rows and columns into
// LDS, padded with zeros to KT = 16 columns.  K_c[i, j] and w_ij are formed
// once per element; the workgroup of chunk 0 also sums a and b.  Tiles off the
// diagonal count twice.  Each workgroup reduces its sums (wave shuffles, then
// the four waves in order) into partial[q * ntiles + tile], q = 0: a, 1: b,
// 2 + p: g_p, 2 + nt + p: h_p -- every slot written exactly once.  With no
// planes (nt = 0) the one chunk gives a and b.
// ka_reduce: dense_reduce.h's reduce_partials, one workgroup per output.
// The grids are functions of the shapes alone and there are no atomics: the
// same bits on every call.
#include "dense_reduce.h"

#define TILE 64
#define KT 16                    // most target columns (LDS rows are padded)

// gridDim.x = ceil(n / NWAVE)
template <typename T>
__device__ __forceinline__ void rows_stage(
    const T *__restrict__ K, int64_t n, int64_t k_lane, int64_t k_col,
    double *__restrict__ r)
{
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t i = (int64_t)blockIdx.x * NWAVE + wid;
    if (i >= n) return;                       // (whole waves only)
    const T *ki = K + i * k_col;
    double t = 0.0;
    for (int64_t l = lane; l < n; l += WAVE) t += (double)ki[l * k_lane];
    t = wave_sum(t);
    if (lane == 0) r[i] = t;
}

extern "C" __global__ __launch_bounds__(BLOCK) void
ka_rows_f32(const float *K, int64_t n, int64_t k_lane, int64_t k_col, double *r)
{
    rows_stage<float>(K, n, k_lane, k_col, r);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
ka_rows_f64(const double *K, int64_t n, int64_t k_lane, int64_t k_col, double *r)
{
    rows_stage<double>(K, n, k_lane, k_col, r);
}

template <typename T, int KC>
__device__ __forceinline__ void planes_stage(
    const T *__restrict__ K, int64_t n, int64_t k_lane, int64_t k_col,
    const double *__restrict__ r, const double *__restrict__ Tc, int kt,
    const T *__restrict__ P, int64_t s_lane, int64_t s_col, int64_t s_k,
    const int64_t *__restrict__ pidx, int nt, int64_t ntiles,
    double *__restrict__ partial)
{
    const int64_t t = blockIdx.x % ntiles;
    const int chunk = (int)(blockIdx.x / ntiles);
    const int k0 = chunk * KC;
    const int nk = max(0, min(KC, nt - k0));
    // tile t -> (I, J), I <= J, column by column: t = J (J + 1) / 2 + I
    int64_t J = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (J * (J + 1) / 2 > t) --J;
    while ((J + 1) * (J + 2) / 2 <= t) ++J;
    const int64_t I = t - J * (J + 1) / 2;

    __shared__ double trow[TILE][KT + 1], tcol[TILE][KT];
    __shared__ double red[NWAVE][2 + 2 * KC];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;

    // the targets of the tile's rows and columns, zeros beyond kt and n
    for (int e = threadIdx.x; e < TILE * KT; e += BLOCK) {
        const int l = e / KT, c = e % KT;
        const int64_t ir = I * TILE + l, jc = J * TILE + l;
        trow[l][c] = (c < kt && ir < n) ? Tc[ir * kt + c] : 0.0;
        tcol[l][c] = (c < kt && jc < n) ? Tc[jc * kt + c] : 0.0;
    }
    // s = sum r, in the order of reduce_partials
    double s = 0.0;
    for (int64_t l = threadIdx.x; l < n; l += BLOCK) s += r[l];
    s = wave_sum(s);
    if (lane == 0) red[wid][0] = s;
    __syncthreads();
    s = 0.0;
    for (int w = 0; w < NWAVE; ++w) s += red[w][0];
    __syncthreads();                          // (red is written again below)

    const double rn = 1.0 / (double)n;
    const double mean = s * rn * rn;
    const int64_t i = I * TILE + lane;
    int64_t off[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk)
        off[kk] = kk < nk ? pidx[k0 + kk] * s_k : 0;
    double a = 0.0, b = 0.0, g[KC], h[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) g[kk] = h[kk] = 0.0;
    if (i < n) {
        double ti[KT];
#pragma unroll
        for (int c = 0; c < KT; ++c) ti[c] = trow[lane][c];
        const double ri = r[i] * rn;
        const T *ki = K + i * k_lane;
        const T *pi = P + i * s_lane;
        const int64_t c0 = J * TILE;
        const int64_t c1 = min(c0 + TILE, n);
        for (int64_t j = c0 + wid; j < c1; j += NWAVE) {
            const double *tj = tcol[j - c0];
            double w = 0.0;
#pragma unroll
            for (int c = 0; c < KT; ++c) w += ti[c] * tj[c];
            const double kc =
                (((double)ki[j * k_col] - ri) - r[j] * rn) + mean;
            a += kc * w;
            b += kc * kc;
            const T *pj = pi + j * s_col;
#pragma unroll
            for (int kk = 0; kk < KC; ++kk)
                if (kk < nk) {
                    const double d = (double)pj[off[kk]];
                    g[kk] += d * w;
                    h[kk] += d * kc;
                }
        }
    }
    const double weight = I == J ? 1.0 : 2.0;
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) {
        red[wid][0] = a;
        red[wid][1] = b;
    }
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) {
        const double x = wave_sum(g[kk]), y = wave_sum(h[kk]);
        if (lane == 0) {
            red[wid][2 + kk] = x;
            red[wid][2 + KC + kk] = y;
        }
    }
    __syncthreads();
    // threads 0, 1: a and b (chunk 0 only); 2 .. 2 + 2 KC: g and h
    const int q = threadIdx.x;
    if (q < 2 + 2 * KC) {
        double x = 0.0;
        for (int w = 0; w < NWAVE; ++w) x += red[w][q];
        int64_t slot = -1;
        if (q < 2) {
            if (chunk == 0) slot = q;
        } else if (q < 2 + KC) {
            if (q - 2 < nk) slot = 2 + k0 + (q - 2);
        } else if (q - 2 - KC < nk) {
            slot = 2 + nt + k0 + (q - 2 - KC);
        }
        if (slot >= 0) partial[slot * ntiles + t] = weight * x;
    }
}

#define PLANES(T, SFX, KC)                                                     \
    extern "C" __global__ __launch_bounds__(BLOCK) void                        \
    ka_planes_##SFX##_k##KC(const T *K, int64_t n, int64_t k_lane,             \
                            int64_t k_col, const double *r, const double *Tc,  \
                            int kt, const T *P, int64_t s_lane, int64_t s_col, \
                            int64_t s_k, const int64_t *pidx, int nt,          \
                            int64_t ntiles, double *partial) {                 \
        planes_stage<T, KC>(K, n, k_lane, k_col, r, Tc, kt, P, s_lane, s_col,  \
                            s_k, pidx, nt, ntiles, partial);                   \
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

// gridDim.x = 2 + 2 nt: out[q] = sum of the ntiles partials of output q
extern "C" __global__ __launch_bounds__(BLOCK) void
ka_reduce(const double *__restrict__ partial, int64_t ntiles,
          double *__restrict__ out)
{
    reduce_partials(partial, ntiles, out);
}
