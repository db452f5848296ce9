// Fused weight-matrix kernels of the Gaussian field regressor (gfr.py; host
// side _field.py).  One call = one block K (Nr x Nc,
// element (r, c) at K[r skr + c skc], float or double, read as it lies); all
// arithmetic double.  Per element, as KernelInducedDistance + RBFOverDistance:
//   d^2 = max(0, -K_rc + half kr_r + half kc_c),  w = exp(-d^2 / 2 sigma^2)
// (w = 0 on r == c of a self block).
// gf_rowsums: s_r = sum_c (w + smoothing), t_r = sum_c (w + smoothing) y_c,
//   optionally Wout = w + smoothing (column-major, leading dimension Nr).
// gf_contract, A_rc = alpha_r + beta_r gamma_c:
//   out[0] = sum A d^2 w sigma^-3
//   out[1 + k] = sum A (-d w sigma^-2) 0.5 / (d + eps)
//                      (-dK_rck + 0.5 dkr_rk + 0.5 dkc_ck),
//   dK_rck = row_r col_c P[r, c, pk[k]] + K_rc (u_rk + v_ck)
//   (row, col, u, v may be NULL; dkr, dkc, u, v column-major double).  The
//   row terms are applied once per row from sum_c coef and sum_c coef K.
// Scheme of lowrank.hip: 64 rows per workgroup (a lane each), columns strided
// over the four waves and gy column sets, KC planes per chunk in registers,
// a shape-only grid and a fixed-order second-stage reduction, no atomics:
// repeated calls give the same bits.
#include "dense_reduce.h"

// d and w of one element, in the order of operations of the host path
__device__ __forceinline__ void field_weight(double k, double kr, double kc,
                                             double half, double s2,
                                             bool diag, double &d, double &w) {
    double t = -k;
    t += half * kr;
    t += half * kc;
    t = fmax(t, 0.0);
    d = sqrt(t);
    w = diag ? 0.0 : exp(-0.5 * (d * d) * s2);
}

template <typename TK>
__device__ __forceinline__ void rowsums_stage1(
    const TK *__restrict__ K, int64_t skr, int64_t skc, int64_t Nr,
    int64_t Nc, const double *__restrict__ kr, const double *__restrict__ kc,
    double half, double s2, double smoothing, int self_block,
    const double *__restrict__ y, double *__restrict__ Wout, int gx, int gy,
    double *__restrict__ ps, double *__restrict__ pt)
{
    const int bx = blockIdx.x % gx, by = blockIdx.x / gx;
    __shared__ double red[2][NWAVE][WAVE];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t r = (int64_t)bx * WAVE + lane;
    double s = 0.0, t = 0.0;
    if (r < Nr) {
        const double krr = kr[r];
        const int64_t cstep = (int64_t)NWAVE * gy;
        for (int64_t c = (int64_t)by * NWAVE + wid; c < Nc; c += cstep) {
            double d, w;
            field_weight((double)K[r * skr + c * skc], krr, kc[c], half, s2,
                         self_block && r == c, d, w);
            const double ws = w + smoothing;
            s += ws;
            if (y) t += ws * y[c];
            if (Wout) Wout[r + Nr * c] = ws;
        }
    }
    red[0][wid][lane] = s;
    red[1][wid][lane] = t;
    __syncthreads();
    if (threadIdx.x < WAVE && r < Nr) {
        double ss = 0.0, tt = 0.0;
        for (int v = 0; v < NWAVE; ++v) {
            ss += red[0][v][lane];
            tt += red[1][v][lane];
        }
        ps[(int64_t)by * Nr + r] = ss;
        pt[(int64_t)by * Nr + r] = tt;
    }
}

#define ROWSUMS(TK, SFX)                                                       \
    extern "C" __global__ __launch_bounds__(BLOCK) void gf_rowsums_##SFX(      \
        const TK *K, int64_t skr, int64_t skc, int64_t Nr, int64_t Nc,         \
        const double *kr, const double *kc, double half, double s2,            \
        double smoothing, int self_block, const double *y, double *Wout,       \
        int gx, int gy, double *ps, double *pt) {                              \
        rowsums_stage1<TK>(K, skr, skc, Nr, Nc, kr, kc, half, s2, smoothing,   \
                           self_block, y, Wout, gx, gy, ps, pt);               \
    }

ROWSUMS(float, f32)
ROWSUMS(double, f64)

// s[r] = sum_b ps[b Nr + r], t likewise; one thread per row, b in order
extern "C" __global__ __launch_bounds__(BLOCK) void
gf_rowsums_reduce(const double *__restrict__ ps, const double *__restrict__ pt,
                  int64_t Nr, int gy, double *__restrict__ s,
                  double *__restrict__ t)
{
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= Nr) return;
    double a = 0.0, b = 0.0;
    for (int k = 0; k < gy; ++k) {
        a += ps[(int64_t)k * Nr + r];
        b += pt[(int64_t)k * Nr + r];
    }
    s[r] = a;
    t[r] = b;
}

template <typename TK, typename TP, int KC>
__device__ __forceinline__ void contract_stage1(
    const TK *__restrict__ K, int64_t skr, int64_t skc, int64_t Nr,
    int64_t Nc, const double *__restrict__ kr, const double *__restrict__ kc,
    const double *__restrict__ dkr, const double *__restrict__ dkc,
    double half, double s2, double s3, double eps, int self_block,
    const double *__restrict__ alpha, const double *__restrict__ beta,
    const double *__restrict__ gamma,
    const TP *__restrict__ P, int64_t spr, int64_t spc, int64_t spk,
    const int *__restrict__ pk, int n,
    const double *__restrict__ row, const double *__restrict__ col,
    const double *__restrict__ u, const double *__restrict__ v,
    int gx, int gy, double *__restrict__ partial)
{
    const int bx = blockIdx.x % gx, by = (blockIdx.x / gx) % gy,
              bz = blockIdx.x / gx / gy;
    __shared__ double red[NWAVE][KC + 1];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t r = (int64_t)bx * WAVE + lane;
    const int k0 = bz * KC;
    const int nk = max(0, min(KC, n - k0));
    int64_t poff[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk)
        poff[kk] = kk < nk ? spk * (int64_t)pk[k0 + kk] : 0;
    double acc[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) acc[kk] = 0.0;
    double sig = 0.0;
    if (r < Nr) {
        const double krr = kr[r], ar = alpha[r], br = beta[r];
        const double rowr = row ? row[r] : 1.0;
        double S1 = 0.0, S2 = 0.0;
        const int64_t cstep = (int64_t)NWAVE * gy;
        for (int64_t c = (int64_t)by * NWAVE + wid; c < Nc; c += cstep) {
            const double kv = (double)K[r * skr + c * skc];
            double d, w;
            field_weight(kv, krr, kc[c], half, s2, self_block && r == c, d, w);
            if (w == 0.0) continue;          // (no plane is read)
            const double A = ar + br * gamma[c];
            sig += A * (d * d * w * s3);
            const double coef = A * ((-d * w * s2) * (0.5 / (d + eps)));
            S1 += coef;
            S2 += coef * kv;
            const double rc = col ? rowr * col[c] : rowr;
            const TP *pp = P + r * spr + c * spc;
#pragma unroll
            for (int kk = 0; kk < KC; ++kk)
                if (kk < nk) {
                    const int64_t k = k0 + kk;
                    double g = 0.5 * dkc[c + Nc * k];
                    if (v) g -= kv * v[c + Nc * k];
                    g -= rc * (double)pp[poff[kk]];
                    acc[kk] += coef * g;
                }
        }
#pragma unroll
        for (int kk = 0; kk < KC; ++kk)
            if (kk < nk) {
                const int64_t k = k0 + kk;
                acc[kk] += 0.5 * dkr[r + Nr * k] * S1;
                if (u) acc[kk] -= u[r + Nr * k] * S2;
            }
    }
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) {
        const double s = wave_sum(acc[kk]);
        if (lane == 0) red[wid][1 + kk] = s;
    }
    {
        const double s = wave_sum(sig);
        if (lane == 0) red[wid][0] = s;
    }
    __syncthreads();
    const int64_t nblk = (int64_t)gx * gy;
    const int64_t blk = bx + (int64_t)gx * by;
    // slot 0 (the sigma column) from the first chunk only
    if (threadIdx.x <= nk && (threadIdx.x > 0 || bz == 0)) {
        double s = 0.0;
        for (int w = 0; w < NWAVE; ++w) s += red[w][threadIdx.x];
        const int64_t slot = threadIdx.x == 0 ? 0 : 1 + k0 + threadIdx.x - 1;
        partial[slot * nblk + blk] = s;
    }
}

#define CONTRACT(TK, TP, SFX, KC)                                              \
    extern "C" __global__ __launch_bounds__(BLOCK) void                        \
    gf_contract_##SFX##_k##KC(                                                 \
        const TK *K, int64_t skr, int64_t skc, int64_t Nr, int64_t Nc,         \
        const double *kr, const double *kc, const double *dkr,                 \
        const double *dkc, double half, double s2, double s3, double eps,      \
        int self_block, const double *alpha, const double *beta,               \
        const double *gamma, const TP *P, int64_t spr, int64_t spc,            \
        int64_t spk, const int *pk, int n, const double *row,                  \
        const double *col, const double *u, const double *v, int gx, int gy,  \
        double *partial) {                                                     \
        contract_stage1<TK, TP, KC>(K, skr, skc, Nr, Nc, kr, kc, dkr, dkc,     \
                                    half, s2, s3, eps, self_block, alpha,      \
                                    beta, gamma, P, spr, spc, spk, pk, n, row, \
                                    col, u, v, gx, gy, partial);               \
    }

#define CONTRACT_CHUNKS(TK, TP, SFX)                                           \
    CONTRACT(TK, TP, SFX, 1)                                                   \
    CONTRACT(TK, TP, SFX, 2)                                                   \
    CONTRACT(TK, TP, SFX, 4)                                                   \
    CONTRACT(TK, TP, SFX, 8)                                                   \
    CONTRACT(TK, TP, SFX, 16)

CONTRACT_CHUNKS(float, float, f32_f32)
CONTRACT_CHUNKS(float, double, f32_f64)
CONTRACT_CHUNKS(double, float, f64_f32)
CONTRACT_CHUNKS(double, double, f64_f64)

// out[j] = sum_b partial[j nblk + b], one workgroup per output (gridDim.x =
// n + 1), b in a fixed order
extern "C" __global__ __launch_bounds__(BLOCK) void
gf_reduce(const double *__restrict__ partial, int64_t nblk,
          double *__restrict__ out)
{
    reduce_partials(partial, nblk, out);
}
