// Blocked subspace iteration for the k largest eigenpairs of the centred
// kernel matrix Kc = H K H, H = I - 1 1^T / n (kpca.py; the host side is
// _subspace.py).  K is n x n, symmetric, float or double,
// contiguous along either index (symmetric: read as it lies); Kc is never
// written.  V, Z, Vr are n x m row-major doubles, m <= 32.  One iteration is
//
//   kpca_apply_* -> kpca_ritz -> kpca_rotate
//
// The block V is stored unnormalised, as the rotate before left it; its column
// statistics travel beside it as per-block partial sums
//   vpart = [sum of squares: m x nvb | sum: m x nvb]
// and every kernel that reads V applies scale_c = 1 / |V_c| on load (col_stats:
// the same fixed-order sum in every workgroup, so the same bits).  Below V
// means that scaled block.
//
// kpca_apply_{f32,f64}_k{KC}: Z = K (V - 1 vmean^T).  A workgroup takes ROWS =
// 16 rows of K and one chunk of KC columns of V; each of its four waves keeps
// RW = 4 rows x KC double accumulators in registers.  The centred chunk of V
// is staged through LDS in tiles of TJ rows, transposed, so that lane l reads
// the entries that belong to its 16 bytes of K (float4 / double2 loads when n
// is a multiple of the vector, single elements otherwise: `n % VEC` decides,
// nothing else).  Each workgroup also writes, for its row block rb,
//   part[rb] = [V^T V (m x m) | V^T Z (m x m) | 1^T Z (m)]
// restricted to its rows (its chunk of the columns of each).
// kpca_ritz: one workgroup.  Sums the row blocks in order, centres G = V^T Z -
// (V^T 1)(1^T Z / n)^T, factors S = V^T V = L L^T, forms T = L^-1 G L^-T and
// diagonalises it by cyclic Jacobi in LDS (round-robin pairs, m / 2 disjoint
// rotations per step, the same order on every call) until off(T) <= eps |T|_F.
// Writes R = L^-T C with the Ritz values in descending order, info = [w (m) |
// (m, for kpca_reduce) | status], cols = [scale | V^T 1 | 1^T Z / n].  Status
// bit 0: S not positive definite (a pivot <= PD_TOL S_jj, or NaN); bit 1: the
// sweep cap was reached.  The status is sticky.
// kpca_rotate: Vr = V R, Yr = (Z - 1 zmean^T) R for RB = 64 rows per
// workgroup; stores Vr and the next block Yr, and per workgroup the partial
// sums rpart = [Yr^2 | Yr | (Yr - w Vr)^2] (each m x nb): the first two are the
// next vpart, the third goes through kpca_reduce to the residual norms.
// kpca_colsum_*: row sums (= column sums) and the diagonal of K.
// kpca_reduce: dense_reduce.h's reduce_partials.
// kpca_project_{f32,f64}_k{KC}: out = (Ks - rowmean - colmean + mean) A for a
// (b, n) cross matrix with any strides, a lane per row of Ks, the n terms split
// over the four waves in order; A's column sums are formed, not assumed zero.
//
// Every grid is a function of the shapes alone, every sum runs in a fixed order
// (wave_sum of dense_reduce.h where a wave adds its lanes) and there are no
// atomics: the same bits on every call.
#include "dense_reduce.h"

#define MMAX 32                  // widest block
#define ROWS 16                  // rows of K per workgroup of kpca_apply
#define RW (ROWS / NWAVE)        // rows per wave, all at once
#define TJ 256                   // rows of V per LDS tile
#define TJP (TJ + 2)             // (padded; rows stay 16-byte aligned)
#define RB 64                    // rows per workgroup of kpca_rotate
#define RSTEP (BLOCK / MMAX)     // rows of kpca_rotate in flight
#define SWEEPS 30                // cap of Jacobi sweeps
#define PD_TOL 1e-13
#define EPS 2.220446049250313e-16

// scale[c] = 1 / |V_c| (0 for a zero or NaN column), vsum[c] = scale[c] 1^T V_c
__device__ __forceinline__ void col_stats(
    const double *__restrict__ vpart, int64_t nvb, int m,
    double *scale, double *vsum)
{
    if ((int)threadIdx.x < m) {
        const double *p = vpart + (int64_t)threadIdx.x * nvb;
        const double *q = vpart + (int64_t)(m + threadIdx.x) * nvb;
        double a = 0.0, b = 0.0;
        for (int64_t k = 0; k < nvb; ++k) {
            a += p[k];
            b += q[k];
        }
        const double s = a > 0.0 ? 1.0 / sqrt(a) : 0.0;
        scale[threadIdx.x] = s;
        vsum[threadIdx.x] = s * b;
    }
}

// the products of one tile: lane l takes columns jj = VEC (l + 64 t) + v
template <typename T, int KC, int VEC>
__device__ __forceinline__ void apply_tile(
    const T *(&row)[RW], int64_t n, int64_t j0,
    double (*Vt)[TJP], int nk, double (&acc)[RW][KC])
{
    const int lane = threadIdx.x % WAVE;
    for (int jj = lane * VEC; jj < TJ; jj += WAVE * VEC) {
        const int64_t j = j0 + jj;
        if (j >= n) break;               // (n % VEC == 0: whole vectors)
        double kv[RW][VEC];
#pragma unroll
        for (int r = 0; r < RW; ++r) load_k<T, VEC>(row[r] + j, kv[r]);
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
            if (kk < nk) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const double vt = Vt[kk][jj + v];
#pragma unroll
                    for (int r = 0; r < RW; ++r) acc[r][kk] += kv[r][v] * vt;
                }
            }
        }
    }
}

// gridDim.x = nrb * ceil(m / KC), nrb = ceil(n / ROWS)
template <typename T, int KC>
__device__ __forceinline__ void apply_stage(
    const T *__restrict__ K, int64_t n, const double *__restrict__ V, int m,
    const double *__restrict__ vpart, int64_t nvb, double *__restrict__ Z,
    double *__restrict__ part)
{
    constexpr int VEC = 16 / sizeof(T);
    __shared__ __attribute__((aligned(16))) double Vt[KC][TJP];
    __shared__ double Vrow[ROWS][MMAX], Zs[ROWS][KC];
    __shared__ double scale[MMAX], vmean[MMAX];
    const int64_t nrb = (n + ROWS - 1) / ROWS;
    const int64_t rb = blockIdx.x % nrb;
    const int c0 = (int)(blockIdx.x / nrb) * KC;
    const int nk = min(KC, m - c0);
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;

    col_stats(vpart, nvb, m, scale, vmean);
    __syncthreads();
    // this block's rows of V, scaled (not centred): for the partial products
    for (int idx = threadIdx.x; idx < ROWS * m; idx += BLOCK) {
        const int r = idx / m, a = idx - r * m;
        const int64_t i = rb * ROWS + r;
        Vrow[r][a] = i < n ? V[i * m + a] * scale[a] : 0.0;
    }
    __syncthreads();
    if ((int)threadIdx.x < m) vmean[threadIdx.x] /= (double)n;

    const T *row[RW];
    bool valid[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const int64_t i = rb * ROWS + wid * RW + r;
        valid[r] = i < n;
        row[r] = K + (valid[r] ? i : 0) * n;     // (in bounds either way)
    }
    double acc[RW][KC];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) acc[r][kk] = 0.0;
    const bool wide = VEC > 1 && n % VEC == 0;

    for (int64_t j0 = 0; j0 < n; j0 += TJ) {
        __syncthreads();                 // (vmean; the tile before is used up)
        for (int idx = threadIdx.x; idx < TJ * nk; idx += BLOCK) {
            const int jj = idx / nk, kk = idx - jj * nk;
            const int64_t j = j0 + jj;
            Vt[kk][jj] = j < n ? V[j * m + c0 + kk] * scale[c0 + kk]
                                     - vmean[c0 + kk] : 0.0;
        }
        __syncthreads();
        if (wide) apply_tile<T, KC, VEC>(row, n, j0, Vt, nk, acc);
        else apply_tile<T, KC, 1>(row, n, j0, Vt, nk, acc);
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) {
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
            const double z = wave_sum(acc[r][kk]);
            if (lane == 0 && kk < nk) {
                Zs[wid * RW + r][kk] = valid[r] ? z : 0.0;
                if (valid[r])
                    Z[(rb * ROWS + wid * RW + r) * m + c0 + kk] = z;
            }
        }
    }
    __syncthreads();
    double *out = part + rb * (2 * (int64_t)m * m + m);
    for (int idx = threadIdx.x; idx < m * nk; idx += BLOCK) {
        const int a = idx / nk, b = idx - a * nk;
        double s = 0.0, g = 0.0;
        for (int r = 0; r < ROWS; ++r) {
            const double va = Vrow[r][a];
            s += va * Vrow[r][c0 + b];
            g += va * Zs[r][b];
        }
        out[a * m + c0 + b] = s;
        out[m * m + a * m + c0 + b] = g;
    }
    if ((int)threadIdx.x < nk) {
        double s = 0.0;
        for (int r = 0; r < ROWS; ++r) s += Zs[r][threadIdx.x];
        out[2 * m * m + c0 + threadIdx.x] = s;
    }
}

#define APPLY(T, SFX, KC)                                                      \
    extern "C" __global__ __launch_bounds__(BLOCK) void                        \
    kpca_apply_##SFX##_k##KC(const T *K, int64_t n, const double *V, int m,    \
                             const double *vpart, int64_t nvb, double *Z,      \
                             double *part) {                                   \
        apply_stage<T, KC>(K, n, V, m, vpart, nvb, Z, part);                   \
    }

APPLY(float, f32, 1)
APPLY(float, f32, 2)
APPLY(float, f32, 4)
APPLY(float, f32, 8)
APPLY(float, f32, 16)
APPLY(double, f64, 1)
APPLY(double, f64, 2)
APPLY(double, f64, 4)
APPLY(double, f64, 8)
APPLY(double, f64, 16)

// sum over the workgroup, the same value in every thread (strided terms, the
// butterfly, then the four waves in order); `red` is reused: two barriers
__device__ __forceinline__ double block_sum(double v, double *red) {
    v = wave_sum(v);
    __syncthreads();
    if (threadIdx.x % WAVE == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < NWAVE; ++w) t += red[w];
    return t;
}

// gridDim.x = 1
extern "C" __global__ __launch_bounds__(BLOCK) void
kpca_ritz(const double *__restrict__ part, int64_t nrb, int m, int64_t n,
          const double *__restrict__ vpart, int64_t nvb,
          double *__restrict__ R, double *__restrict__ info,
          double *__restrict__ cols)
{
    __shared__ double Tm[MMAX][MMAX + 1], Lm[MMAX][MMAX + 1],
        Cm[MMAX][MMAX + 1];
    __shared__ double scale[MMAX], vsum[MMAX], zmean[MMAX], sdiag[MMAX],
        tmp[MMAX], wv[MMAX], cs[MMAX / 2][2], red[NWAVE];
    __shared__ int pq[MMAX / 2][2], perm[MMAX], flag;
    const int t = threadIdx.x;
    const int mm = m * m;
    const int64_t rec = 2 * (int64_t)mm + m;

    col_stats(vpart, nvb, m, scale, vsum);
    for (int idx = t; idx < mm; idx += BLOCK) {
        double s = 0.0, g = 0.0;
        for (int64_t rb = 0; rb < nrb; ++rb) {
            s += part[rb * rec + idx];
            g += part[rb * rec + mm + idx];
        }
        Lm[idx / m][idx % m] = s;
        Tm[idx / m][idx % m] = g;
        Cm[idx / m][idx % m] = idx / m == idx % m ? 1.0 : 0.0;
    }
    if (t < m) {
        double z = 0.0;
        for (int64_t rb = 0; rb < nrb; ++rb) z += part[rb * rec + 2 * mm + t];
        zmean[t] = z / (double)n;
    }
    if (t == 0) flag = 0;
    __syncthreads();
    if (t < m) {
        cols[t] = scale[t];
        cols[m + t] = vsum[t];
        cols[2 * m + t] = zmean[t];
        sdiag[t] = Lm[t][t];
    }
    // G = V^T Z - (V^T 1) zmean^T, symmetrised (thread (a, b), a <= b, owns
    // both entries)
    for (int idx = t; idx < mm; idx += BLOCK) {
        const int a = idx / m, b = idx % m;
        if (a > b) continue;
        const double g = 0.5 * ((Tm[a][b] - vsum[a] * zmean[b])
                                + (Tm[b][a] - vsum[b] * zmean[a]));
        Tm[a][b] = g;
        Tm[b][a] = g;
    }
    __syncthreads();

    // S = L L^T in place (left-looking; the lower triangle of Lm)
    for (int j = 0; j < m; ++j) {
        if (t >= j && t < m) {
            double v = Lm[t][j];
            for (int k = 0; k < j; ++k) v -= Lm[t][k] * Lm[j][k];
            tmp[t] = v;
        }
        __syncthreads();
        if (t >= j && t < m) {
            const double d = tmp[j];
            if (t == j) {
                if (!(d > PD_TOL * sdiag[j])) flag = 1;
                Lm[j][j] = sqrt(d);
            } else {
                Lm[t][j] = tmp[t] / sqrt(d);
            }
        }
        __syncthreads();
    }
    if (flag) {                           // (uniform)
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int idx = t; idx < mm; idx += BLOCK) R[idx] = nan;
        if (t < m) info[t] = nan;
        if (t == 0) info[2 * m] = (double)((int)info[2 * m] | 1);
        return;
    }

    // T = L^-1 G L^-T: forward substitution down the columns, twice
    for (int pass = 0; pass < 2; ++pass) {
        if (t < m) {
            for (int i = 0; i < m; ++i) {
                double x = Tm[i][t];
                for (int k = 0; k < i; ++k) x -= Lm[i][k] * Tm[k][t];
                Tm[i][t] = x / Lm[i][i];
            }
        }
        __syncthreads();
        for (int idx = t; idx < mm; idx += BLOCK) {     // transpose
            const int a = idx / m, b = idx % m;
            if (a < b) {
                const double u = Tm[a][b];
                Tm[a][b] = Tm[b][a];
                Tm[b][a] = u;
            }
        }
        __syncthreads();
    }
    for (int idx = t; idx < mm; idx += BLOCK) {
        const int a = idx / m, b = idx % m;
        if (a < b) {
            const double u = 0.5 * (Tm[a][b] + Tm[b][a]);
            Tm[a][b] = u;
            Tm[b][a] = u;
        }
    }
    __syncthreads();

    // cyclic Jacobi, round-robin: M players (m rounded up to even), M - 1
    // steps of M / 2 disjoint pairs per sweep
    const int M = (m + 1) & ~1, half = M / 2;
    bool capped = false;
    for (int sweep = 0;; ++sweep) {
        double off = 0.0, tot = 0.0;
        for (int idx = t; idx < mm; idx += BLOCK) {
            const double u = Tm[idx / m][idx % m];
            tot += u * u;
            if (idx / m != idx % m) off += u * u;
        }
        off = block_sum(off, red);
        tot = block_sum(tot, red);
        if (!(off > EPS * EPS * tot)) break;
        if (sweep == SWEEPS) {
            capped = true;
            break;
        }
        for (int step = 0; step < M - 1; ++step) {
            if (t < half) {
                int p = t == 0 ? M - 1 : (step + t) % (M - 1);
                int q = t == 0 ? step : (step - t + (M - 1)) % (M - 1);
                if (p > q) { const int u = p; p = q; q = u; }
                double c = 1.0, s = 0.0;
                if (q < m) {
                    const double apq = Tm[p][q];
                    if (apq != 0.0) {
                        const double th = (Tm[q][q] - Tm[p][p]) / (2.0 * apq);
                        const double tt = (th >= 0.0 ? 1.0 : -1.0)
                            / (fabs(th) + sqrt(th * th + 1.0));
                        c = 1.0 / sqrt(tt * tt + 1.0);
                        s = tt * c;
                    }
                } else {
                    q = p;                // (the bye of an odd m)
                }
                pq[t][0] = p; pq[t][1] = q;
                cs[t][0] = c; cs[t][1] = s;
            }
            __syncthreads();
            // columns: T <- T J, C <- C J
            for (int idx = t; idx < half * m; idx += BLOCK) {
                const int h = idx / m, i = idx % m;
                const int p = pq[h][0], q = pq[h][1];
                if (p == q) continue;
                const double c = cs[h][0], s = cs[h][1];
                const double tp = Tm[i][p], tq = Tm[i][q];
                Tm[i][p] = c * tp - s * tq;
                Tm[i][q] = s * tp + c * tq;
                const double cp = Cm[i][p], cq = Cm[i][q];
                Cm[i][p] = c * cp - s * cq;
                Cm[i][q] = s * cp + c * cq;
            }
            __syncthreads();
            // rows: T <- J^T T
            for (int idx = t; idx < half * m; idx += BLOCK) {
                const int h = idx / m, j = idx % m;
                const int p = pq[h][0], q = pq[h][1];
                if (p == q) continue;
                const double c = cs[h][0], s = cs[h][1];
                const double tp = Tm[p][j], tq = Tm[q][j];
                Tm[p][j] = c * tp - s * tq;
                Tm[q][j] = s * tp + c * tq;
            }
            __syncthreads();
            if (t < half && pq[t][0] != pq[t][1] && cs[t][1] != 0.0) {
                Tm[pq[t][0]][pq[t][1]] = 0.0;
                Tm[pq[t][1]][pq[t][0]] = 0.0;
            }
            __syncthreads();
        }
    }

    // descending order (stable), then R = L^-T C P by back substitution
    if (t == 0) {
        for (int j = 0; j < m; ++j) {
            const double w = Tm[j][j];
            int k = j;
            while (k > 0 && wv[k - 1] < w) {
                wv[k] = wv[k - 1];
                perm[k] = perm[k - 1];
                --k;
            }
            wv[k] = w;
            perm[k] = j;
        }
    }
    __syncthreads();
    if (t < m) {
        const int src = perm[t];
        for (int i = m - 1; i >= 0; --i) {
            double x = Cm[i][src];
            for (int k = i + 1; k < m; ++k) x -= Lm[k][i] * Tm[k][t];
            Tm[i][t] = x / Lm[i][i];
        }
    }
    __syncthreads();
    for (int idx = t; idx < mm; idx += BLOCK) R[idx] = Tm[idx / m][idx % m];
    if (t < m) info[t] = wv[t];
    if (t == 0 && capped) info[2 * m] = (double)((int)info[2 * m] | 2);
}

// gridDim.x = nb = ceil(n / RB)
extern "C" __global__ __launch_bounds__(BLOCK) void
kpca_rotate(const double *__restrict__ V, const double *__restrict__ Z,
            int64_t n, int m, const double *__restrict__ R,
            const double *__restrict__ info, const double *__restrict__ cols,
            double *__restrict__ Vr, double *__restrict__ Vnext,
            double *__restrict__ rpart)
{
    __shared__ double Rm[MMAX][MMAX + 1], Vs[RSTEP][MMAX], Zs[RSTEP][MMAX];
    __shared__ double red[3][RSTEP][MMAX];
    const int c = threadIdx.x % MMAX, r = threadIdx.x / MMAX;
    const int64_t nb = gridDim.x;
    for (int idx = threadIdx.x; idx < m * m; idx += BLOCK)
        Rm[idx / m][idx % m] = R[idx];
    const bool on = c < m;
    const double sc = on ? cols[c] : 0.0, zm = on ? cols[2 * m + c] : 0.0;
    const double w = on ? info[c] : 0.0;
    double n2 = 0.0, sm = 0.0, r2 = 0.0;
    for (int it = 0; it < RB / RSTEP; ++it) {
        const int64_t i = (int64_t)blockIdx.x * RB + it * RSTEP + r;
        const bool in = on && i < n;
        __syncthreads();                 // (Rm; the rows before are used up)
        Vs[r][c] = in ? V[i * m + c] * sc : 0.0;
        Zs[r][c] = in ? Z[i * m + c] - zm : 0.0;
        __syncthreads();
        if (in) {
            double vr = 0.0, yr = 0.0;
            for (int a = 0; a < m; ++a) {
                const double ra = Rm[a][c];
                vr += Vs[r][a] * ra;
                yr += Zs[r][a] * ra;
            }
            Vr[i * m + c] = vr;
            Vnext[i * m + c] = yr;
            const double d = yr - w * vr;
            n2 += yr * yr;
            sm += yr;
            r2 += d * d;
        }
    }
    red[0][r][c] = n2;
    red[1][r][c] = sm;
    red[2][r][c] = r2;
    __syncthreads();
    if (r < 3 && on) {                    // (thread (kind, c))
        double s = 0.0;
        for (int k = 0; k < RSTEP; ++k) s += red[r][k][c];
        rpart[((int64_t)r * m + c) * nb + blockIdx.x] = s;
    }
}

// stat = [row sums (n) | diagonal (n)]; gridDim.x = ceil(n / NWAVE)
template <typename T>
__device__ __forceinline__ void colsum_stage(
    const T *__restrict__ K, int64_t n, double *__restrict__ stat)
{
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t i = (int64_t)blockIdx.x * NWAVE + wid;
    if (i >= n) return;                       // (whole waves only)
    const T *ki = K + i * n;
    double s = 0.0;
    for (int64_t j = lane; j < n; j += WAVE) s += (double)ki[j];
    s = wave_sum(s);
    if (lane == 0) {
        stat[i] = s;
        stat[n + i] = (double)ki[i];
    }
}

extern "C" __global__ __launch_bounds__(BLOCK) void
kpca_colsum_f32(const float *K, int64_t n, double *stat) {
    colsum_stage<float>(K, n, stat);
}

extern "C" __global__ __launch_bounds__(BLOCK) void
kpca_colsum_f64(const double *K, int64_t n, double *stat) {
    colsum_stage<double>(K, n, stat);
}

// out[j] = sum of the nblk values partial[j nblk ...], fixed order
extern "C" __global__ __launch_bounds__(BLOCK) void
kpca_reduce(const double *__restrict__ partial, int64_t nblk,
            double *__restrict__ out)
{
    reduce_partials(partial, nblk, out);
}

// Ks[c s_c + i s_i]; A (n, k) row-major; out (b, k) row-major;
// gridDim.x = ceil(b / WAVE)
template <typename T, int KC>
__device__ __forceinline__ void project_stage(
    const T *__restrict__ Ks, int64_t b, int64_t n, int64_t s_c, int64_t s_i,
    const double *__restrict__ A, int k, const double *__restrict__ colmean,
    double gmean, double *__restrict__ out)
{
    __shared__ double sh[NWAVE][KC + 1][WAVE], asl[NWAVE][KC];
    const int lane = threadIdx.x % WAVE, wid = threadIdx.x / WAVE;
    const int64_t c = (int64_t)blockIdx.x * WAVE + lane;
    const int64_t span = (n + NWAVE - 1) / NWAVE;
    const int64_t i0 = wid * span, i1 = min(n, i0 + span);
    const T *p = Ks + (c < b ? c : 0) * s_c;
    double acc[KC], asum[KC], rs = 0.0;
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) acc[kk] = asum[kk] = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
        const double ks = (double)p[i * s_i], d = ks - colmean[i];
        rs += ks;
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) {
            if (kk < k) {
                const double a = A[i * k + kk];
                acc[kk] += d * a;
                asum[kk] += a;
            }
        }
    }
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) {
        sh[wid][kk][lane] = acc[kk];
        if (lane == 0) asl[wid][kk] = asum[kk];
    }
    sh[wid][KC][lane] = rs;
    __syncthreads();
    if (wid == 0 && c < b) {
        double rt = 0.0;
        for (int w = 0; w < NWAVE; ++w) rt += sh[w][KC][lane];
        const double shift = rt / (double)n - gmean;
        for (int kk = 0; kk < k; ++kk) {
            double s = 0.0, a = 0.0;
            for (int w = 0; w < NWAVE; ++w) {
                s += sh[w][kk][lane];
                a += asl[w][kk];
            }
            out[c * k + kk] = s - shift * a;
        }
    }
}

#define PROJECT(T, SFX, KC)                                                    \
    extern "C" __global__ __launch_bounds__(BLOCK) void                        \
    kpca_project_##SFX##_k##KC(const T *Ks, int64_t b, int64_t n,              \
                               int64_t s_c, int64_t s_i, const double *A,      \
                               int k, const double *colmean, double gmean,     \
                               double *out) {                                  \
        project_stage<T, KC>(Ks, b, n, s_c, s_i, A, k, colmean, gmean, out);   \
    }

PROJECT(float, f32, 1)
PROJECT(float, f32, 2)
PROJECT(float, f32, 4)
PROJECT(float, f32, 8)
PROJECT(float, f32, 16)
PROJECT(double, f64, 1)
PROJECT(double, f64, 2)
PROJECT(double, f64, 4)
PROJECT(double, f64, 8)
PROJECT(double, f64, 16)
