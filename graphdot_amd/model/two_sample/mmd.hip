// The sums of the kernel two-sample test (mmd.py; the host side is _mmd.py;
// Gretton et al. 2012).  K is the (n, n) symmetric Gram
// matrix of the pooled sample, Z the (rows, n) bytes 0 and 1 of the splits
// (row 0 the observed one, the others its permutations; bit 0 of a byte is
// read), r = K 1 and d = diag K.
// For every split z the launches give
//
//   q = z^T K z        u = z^T r        dz = z^T d
//
// and, for the weights s of the observed split, the witness w = K s.  K is
// read in the type the solver stored it in, float or double, as it lies: the
// element (i, j) at K[i k_lane + j k_col] (the matrix is symmetric; the host
// picks as the lane axis the one with the smaller stride).  Every sum is
// double.
//
// mmd_rows_*: one wave per index i: r_i, d_i and w_i (lanes strided over the
// row, then the butterfly).
// mmd_forms_*_k{KC}: the pass over K.  One workgroup of four waves per strip I
// of 64 rows and group of 64 KC splits.  For J = I, I + 1, ... the 64 x 64
// tile K[I, J] is staged once in LDS as doubles (zeros beyond n; rows padded
// to LT = 65 doubles: the operand reads of a half wave fall into 32 distinct
// bank pairs), and next to it the 64 bytes of each of the 64 KC splits at the
// tile's columns (zeros beyond n and beyond the last split; 80 bytes apart).
// The tile is used for all KC chunks of 64 splits.  Wave w owns the splits
// 16 w ... 16 w + 15 of a chunk and forms Y = K_IJ Z_J^T, 64 x 16, as four
// 16 x 16 blocks on v_mfma_f64_16x16x4_f64, the B operand being the byte of Z
// widened to double.  The k index of the instruction is free to name: at step
// s, lane group g = lane >> 4 stands for column 16 g + s of the tile, so that
// a lane reads its 16 consecutive bytes of a split in one piece.  Element e of
// block rb in lane l is row 16 rb + (l >> 4) + 4 e of the strip for the split
// l & 15 (the f64 C/D map).  It is added, where z has a one at that row (a
// 16-bit mask per lane and chunk, taken from the staged bytes of the diagonal
// tile), with weight 2 for J > I, to the one running double the lane keeps
// per chunk; after the last J the four lane groups are added as (g0 + g1) +
// (g2 + g3) and partial[I rows + b] is stored.  Every slot is written exactly
// once.  LDS: 33 280 + 5 120 KC bytes; KC is 1, 2 or 4 (measured: larger
// chunks leave one workgroup per CU and are slower).
// mmd_reduce: one wave per split b: q_b = sum_I partial[I rows + b] in
// ascending I; u_b and dz_b over the ones of its row (lanes strided, then the
// butterfly).
//
// What a split's three sums are made of, and in which order, depends on that
// split and on n alone -- not on its row b, on the number of rows or on KC:
// the products by 0, 1 and 2 are exact, and an MFMA column is a function of
// its own B column.  Identical rows give identical bits, and so do two calls.
#include "dense_reduce.h"

#define TILE 64
#define LT 65                   // doubles per staged row
#define ZP 80                   // bytes per staged split: 64 and a pad of 16

typedef double v4d __attribute__((ext_vector_type(4)));

// gridDim.x = ceil(n / NWAVE)
template <typename T>
__device__ __forceinline__ void rows_stage(
    const T *__restrict__ K, int64_t n, int64_t k_lane, int64_t k_col,
    const double *__restrict__ s, double *__restrict__ r,
    double *__restrict__ d, double *__restrict__ w)
{
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t i = (int64_t)blockIdx.x * NWAVE + wid;
    if (i >= n) return;                       // (whole waves only)
    const T *ki = K + i * k_col;
    double t = 0.0, v = 0.0;
    for (int64_t l = lane; l < n; l += WAVE) {
        const double x = (double)ki[l * k_lane];
        t += x;
        v += x * s[l];
    }
    t = wave_sum(t);
    v = wave_sum(v);
    if (lane == 0) {
        r[i] = t;
        d[i] = (double)ki[i * k_lane];
        w[i] = v;
    }
}

extern "C" __global__ __launch_bounds__(BLOCK) void
mmd_rows_f32(const float *K, int64_t n, int64_t k_lane, int64_t k_col,
             const double *s, double *r, double *d, double *w)
{
    rows_stage<float>(K, n, k_lane, k_col, s, r, d, w);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
mmd_rows_f64(const double *K, int64_t n, int64_t k_lane, int64_t k_col,
             const double *s, double *r, double *d, double *w)
{
    rows_stage<double>(K, n, k_lane, k_col, s, r, d, w);
}

// gridDim.x = nb * groups, groups = ceil(rows / (64 KC)), nb = ceil(n / TILE);
// the group is the fast index: workgroups start in the order of their
// strips, the longest first
template <typename T, int KC>
__device__ __forceinline__ void forms_stage(
    const T *__restrict__ K, int64_t n, int64_t k_lane, int64_t k_col,
    const uint8_t *__restrict__ Z, int64_t rows, int64_t nb,
    double *__restrict__ partial)
{
    const int64_t groups = gridDim.x / nb;
    const int64_t I = blockIdx.x / groups;
    const int64_t first = (int64_t)(blockIdx.x % groups) * (WAVE * KC);
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int c = lane & 15, g = lane >> 4;
    __shared__ double tile[TILE][LT];
    __shared__ __attribute__((aligned(16))) uint8_t zs[WAVE * KC][ZP];

    // this lane's split in chunk kc is b0 + 64 kc; bit 4 rb + e of its mask
    // is z at the row of accumulator element e of block rb (read from the
    // staged bytes of the diagonal tile, the first one)
    const int64_t b0 = first + 16 * wid + c;
    unsigned mask[KC];
    double acc[KC];
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
        mask[kc] = 0u;
        acc[kc] = 0.0;
    }

    for (int64_t J = I; J < nb; ++J) {
        __syncthreads();                      // (the last tile has been read)
        {
            // (loads at clamped, valid indices, all in flight together; what
            // lies beyond n becomes zero afterwards)
            double v[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int e = threadIdx.x + BLOCK * q;
                const int64_t i = min(I * TILE + (e & 63), n - 1);
                const int64_t j = min(J * TILE + (e >> 6), n - 1);
                v[q] = (double)K[i * k_lane + j * k_col];
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int e = threadIdx.x + BLOCK * q, a = e & 63, bb = e >> 6;
                tile[a][bb] = (I * TILE + a < n && J * TILE + bb < n)
                    ? v[q] : 0.0;
            }
        }
        // the bytes of the 64 KC splits at the tile's columns (zero beyond n
        // and beyond the last split): a thread brings 16 of them, the
        // quarter sg of split rl, as the five aligned words that hold them,
        // shifted into place by v_alignbyte.  Every word is loaded from an
        // aligned address that holds at least one byte of Z: an address
        // beyond the last such word is clamped to it, and what it would have
        // held lies beyond n and is masked.  All 5 KC loads are in flight
        // together (the empty asm keeps the compiler from waiting for each
        // load before it issues the next)
        {
            const int sg = threadIdx.x & 3;
            const int64_t jw = J * TILE + 16 * sg;
            // (offsets from Z, so that the loads stay global ones)
            const int64_t zb = (int64_t)((uintptr_t)Z & 3);
            const int64_t last = ((zb + rows * n - 1) & ~(int64_t)3) - zb;
            uint32_t v[5 * KC];
            unsigned sh[KC];
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
                const int rl = WAVE * kc + (threadIdx.x >> 2);
                const int64_t at = min(first + rl, rows - 1) * n + jw;
                sh[kc] = (unsigned)((zb + at) & 3);
#pragma unroll
                for (int k = 0; k < 5; ++k)
                    v[5 * kc + k] = *(const uint32_t *)(
                        Z + min(at - sh[kc] + 4 * k, last));
            }
#pragma unroll
            for (int kc = 0; kc < KC; ++kc)
                asm volatile("" : "+v"(v[5 * kc]), "+v"(v[5 * kc + 1]),
                             "+v"(v[5 * kc + 2]), "+v"(v[5 * kc + 3]),
                             "+v"(v[5 * kc + 4]));
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
                const int rl = WAVE * kc + (threadIdx.x >> 2);
                uint32_t w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int64_t left = n - (jw + 4 * k);     // (below n)
                    const uint32_t keep = first + rl >= rows || left <= 0
                        ? 0u : left >= 4 ? 0x01010101u
                        : 0x01010101u & ((1u << (8 * (int)left)) - 1u);
                    w[k] = __builtin_amdgcn_alignbyte(
                        v[5 * kc + k + 1], v[5 * kc + k], sh[kc]) & keep;
                }
                *(uint4 *)&zs[rl][16 * sg] =
                    make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        __syncthreads();
        if (J == I) {
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
                const uint8_t *zl = zs[WAVE * kc + 16 * wid + c];
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    mask[kc] |= (unsigned)zl[16 * (q >> 2) + 4 * (q & 3) + g]
                        << q;
            }
        }
        const double weight = J == I ? 1.0 : 2.0;
        const double *const a0 = &tile[c][16 * g];
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
            if (first + WAVE * kc >= rows) continue;      // (all four waves)
            const uint4 zz =
                *(const uint4 *)&zs[WAVE * kc + 16 * wid + c][16 * g];
            const uint32_t zw[4] = {zz.x, zz.y, zz.z, zz.w};
            double zb[16];
#pragma unroll
            for (int s = 0; s < 16; ++s)
                zb[s] = (zw[s >> 2] >> (8 * (s & 3)) & 1u) ? 1.0 : 0.0;
            v4d y[4];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) y[rb] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 16; ++s)
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
                    y[rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                        a0[16 * rb * LT + s], zb[s], y[rb], 0, 0, 0);
            double t = acc[kc];
#pragma unroll
            for (int q = 0; q < 16; ++q)
                t += (mask[kc] >> q & 1u) ? weight * y[q >> 2][q & 3] : 0.0;
            acc[kc] = t;
        }
    }

#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
        if (first + WAVE * kc >= rows) continue;
        const int64_t b = b0 + WAVE * kc;
        double t = acc[kc];
        t += __shfl_xor(t, 16, WAVE);
        t += __shfl_xor(t, 32, WAVE);
        if (g == 0 && b < rows) partial[I * rows + b] = t;
    }
}

#define FORMS(T, SFX, KC)                                                      \
    extern "C" __global__ __launch_bounds__(BLOCK)                             \
    __attribute__((amdgpu_waves_per_eu(1, 2))) void                            \
    mmd_forms_##SFX##_k##KC(const T *K, int64_t n, int64_t k_lane,             \
                            int64_t k_col, const uint8_t *Z, int64_t rows,     \
                            int64_t nb, double *partial) {                     \
        forms_stage<T, KC>(K, n, k_lane, k_col, Z, rows, nb, partial);         \
    }

FORMS(float, f32, 1)
FORMS(float, f32, 2)
FORMS(float, f32, 4)
FORMS(double, f64, 1)
FORMS(double, f64, 2)
FORMS(double, f64, 4)

// gridDim.x = ceil(rows / NWAVE): out[3 b ...] = q_b, u_b, dz_b
extern "C" __global__ __launch_bounds__(BLOCK) void
mmd_reduce(const double *__restrict__ partial, int64_t nb,
           const uint8_t *__restrict__ Z, int64_t rows, int64_t n,
           const double *__restrict__ r, const double *__restrict__ d,
           double *__restrict__ out)
{
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t b = (int64_t)blockIdx.x * NWAVE + wid;
    if (b >= rows) return;                    // (whole waves only)
    const uint8_t *zb = Z + b * n;
    double u = 0.0, dz = 0.0;
    for (int64_t l = lane; l < n; l += WAVE)
        if (zb[l]) {
            u += r[l];
            dz += d[l];
        }
    u = wave_sum(u);
    dz = wave_sum(dz);
    if (lane == 0) {
        double q = 0.0;
        for (int64_t I = 0; I < nb; ++I) q += partial[I * rows + b];
        out[3 * b] = q;
        out[3 * b + 1] = u;
        out[3 * b + 2] = dz;
    }
}
