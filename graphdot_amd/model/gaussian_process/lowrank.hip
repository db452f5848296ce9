// Gradient contraction of the Nystrom low-rank regressor (nystrom.py; the
// host side is _lowrank.py):
//
//   out[k] = sum_{r, c} W[r, c] * P[rows[r], c, k]          k = 0 .. nt - 1
//
// P: the kernel's gradient planes (N x M x nt, column-major: element (i, c, k)
// at i + N c + N M k) in the type the solver stored them in, float or double,
// read as they lie -- no double copy first.  W: double, Nr x M, column-major
// with leading dimension ldw.  rows: Nr row indices into P (NULL: Nr == N,
// row r of W is row r of P).  Every product and sum is double.
//
// One pass over P.  lr_contract_* (stage 1): a workgroup of four waves takes
// 64 consecutive rows (one per lane) and a strided set of columns (one column
// per wave at a time); for each (row, column) it loads W once and then the
// same element of KC planes, with KC accumulators in registers, so W is read
// once per chunk of KC planes (once in all when nt <= 16).  The 1-D grid is
// gx row tiles x gy column sets x the chunks, so every plane of a call is in
// one launch.  An element whose W is zero loads no plane.  Each workgroup
// reduces its KC sums (wave shuffles, then the four waves in order) into
// partial[k * nblk + block].
// lr_reduce (stage 2): one workgroup per plane sums its nblk partials in a
// fixed order.  The grid is a function of the shapes alone and there are no
// atomics, so the result is the same bits on every call.
#include "dense_reduce.h"

template <typename T, int KC>
__device__ __forceinline__ void contract_stage1(
    const T *__restrict__ P, int64_t N, int64_t M, int nt,
    const double *__restrict__ W, int64_t ldw,
    const int64_t *__restrict__ rows, int64_t Nr, int gx, int gy,
    double *__restrict__ partial)
{
    const int bx = blockIdx.x % gx, by = (blockIdx.x / gx) % gy,
              bz = blockIdx.x / gx / gy;
    __shared__ double red[NWAVE][KC];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t r = (int64_t)bx * WAVE + lane;
    const int k0 = bz * KC;
    const int nk = min(KC, nt - k0);
    const int64_t plane = N * M;
    double acc[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) acc[kk] = 0.0;
    if (r < Nr) {
        const int64_t i = rows ? rows[r] : r;
        const T *p = P + i + plane * k0;
        const double *w = W + r;
        const int64_t cstep = (int64_t)NWAVE * gy;
        for (int64_t c = (int64_t)by * NWAVE + wid; c < M; c += cstep) {
            const double wv = w[ldw * c];
            if (wv != 0.0) {
                const T *pc = p + N * c;
#pragma unroll
                for (int kk = 0; kk < KC; ++kk)
                    if (kk < nk) acc[kk] += wv * (double)pc[plane * kk];
            }
        }
    }
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) {
        const double s = wave_sum(acc[kk]);
        if (lane == 0) red[wid][kk] = s;
    }
    __syncthreads();
    if (threadIdx.x < nk) {
        double s = 0.0;
        for (int w = 0; w < NWAVE; ++w) s += red[w][threadIdx.x];
        const int64_t nblk = (int64_t)gx * gy;
        partial[(k0 + threadIdx.x) * nblk + bx + (int64_t)gx * by] = s;
    }
}

#define STAGE1(T, SFX, KC)                                                     \
    extern "C" __global__ __launch_bounds__(BLOCK) void                        \
    lr_contract_##SFX##_k##KC(const T *P, int64_t N, int64_t M, int nt,        \
                              const double *W, int64_t ldw,                    \
                              const int64_t *rows, int64_t Nr, int gx, int gy, \
                              double *partial) {                               \
        contract_stage1<T, KC>(P, N, M, nt, W, ldw, rows, Nr, gx, gy,          \
                               partial);                                       \
    }

STAGE1(float, f32, 1)
STAGE1(float, f32, 2)
STAGE1(float, f32, 4)
STAGE1(float, f32, 8)
STAGE1(float, f32, 16)
STAGE1(double, f64, 1)
STAGE1(double, f64, 2)
STAGE1(double, f64, 4)
STAGE1(double, f64, 8)
STAGE1(double, f64, 16)

// out[k] = sum_b partial[k nblk + b], one workgroup per plane (gridDim.x = nt)
extern "C" __global__ __launch_bounds__(BLOCK) void
lr_reduce(const double *__restrict__ partial, int64_t nblk,
          double *__restrict__ out)
{
    reduce_partials(partial, nblk, out);
}
