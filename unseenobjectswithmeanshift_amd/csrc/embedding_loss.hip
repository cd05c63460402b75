// EmbeddingLoss (the UCN clustering loss, lib/networks/embedding.py) on per-(image, cluster) sums: NCHW fp32, gfx950.
//
// Forward, six launches on one stream:
//   stats     grid (G, B)  one read of x and the labels: per-workgroup partial tables of S = sum x_p and n per cluster
//   sum       grid (., B)  the partials summed in workgroup order
//   finish    grid (B)     K, the centres, the K x K inter term and its gradient with respect to the centres
//   dist      grid (G, B)  second read of x: d_p, partial D = sum d^2, N = #{d > alpha}, T = sum d_p x_p (cosine), strays
//   sum       grid (., B)  those partials summed in workgroup order
//   finalize  grid (B)     the three losses, the branch flag, the per-cluster coefficients and the centre-path vectors
// Backward, one launch: one read of x and the labels, one write of grad_x.
//
// Determinism: a workgroup's pixel range depends on the shape alone; inside a workgroup every wave owns a private LDS table
// (no LDS or global floating-point atomics), the waves' tables are added in wave order, the workgroups' partials in workgroup
// order.  Lanes own consecutive pixels and loop over the channels (H W apart), so every load is coalesced; the labels of a wave
// are reduced per DISTINCT label across the lanes (labels are spatially coherent: one to three per wave).
#include "common.h"

namespace {

using msm::wave_sum;

constexpr int EL_MAX_TABLE = 16384;      // max_clusters * C floats
constexpr int EL_MAX_K = 1024;
constexpr int EL_MAX_G = 2048;
constexpr int EL_HDR = 16;               // workspace header words: [0] a_stray (float)
constexpr int EL_INFO_HDR = 4;           // info: [0] K, [1] status, [2] branch flag, [3] 0, then n [B][Kt], N [B][Kt]

struct Plan {
    int W;            // waves per workgroup of the two pixel passes
    int G;            // workgroups per image
    int chunk;        // pixels per workgroup (a multiple of 64 W)
    int pstride;      // words of one workgroup's partial: T [Kt C], count [Kt] int, D [Kt], misc [4]
    int64_t o_wginfo, o_nrm, o_coef, o_irow, o_D, o_stray, o_S, o_mu, o_T, o_VI, o_VE, o_H, o_part, total;   // in words
};

Plan plan(int B, int C, int HW, int Kt) {
    Plan P;
    const int tbl = Kt * C + 2 * Kt;                       // words of one wave's LDS table
    P.W = (int64_t)tbl * 4 * 4 <= 72 * 1024 ? 4 : ((int64_t)tbl * 4 * 2 <= 72 * 1024 ? 2 : 1);   // private tables of all waves within 72 KiB, else one wave
    const int per = 64 * P.W;
    int G = msm::cdiv(HW, (int64_t)per * 4);
    const int cap = EL_MAX_G / B > 1 ? EL_MAX_G / B : 1;
    G = G < 1 ? 1 : (G > cap ? cap : G);
    P.chunk = msm::cdiv(msm::cdiv(HW, G), per) * per;
    P.G = msm::cdiv(HW, P.chunk);
    P.pstride = Kt * C + 2 * Kt + 4;
    int64_t o = EL_HDR;
    const int64_t BK = (int64_t)B * Kt, BKC = BK * C;
    P.o_wginfo = o, o += (int64_t)B * P.G * 4;
    P.o_nrm = o, o += BK;
    P.o_coef = o, o += BK;
    P.o_irow = o, o += BK;
    P.o_D = o, o += BK;
    P.o_stray = o, o += (int64_t)B * 2;
    P.o_S = o, o += BKC;
    P.o_mu = o, o += BKC;
    P.o_T = o, o += BKC;
    P.o_VI = o, o += BKC;
    P.o_VE = o, o += BKC;
    P.o_H = o, o += BK * Kt;
    P.o_part = o, o += (int64_t)B * P.G * P.pstride;
    P.total = o;
    return P;
}

bool shape_ok(int B, int C, int HW, int Kt) {
    return B > 0 && B <= 65535 && C >= 1 && HW >= 1 && Kt >= 1 && Kt <= EL_MAX_K && (int64_t)Kt * C <= EL_MAX_TABLE;
}

// >= 0: the cluster; -1: labelled but of no cluster (a non-integer label, or one the table cannot hold); -2: not labelled
__device__ __forceinline__ int cluster_of(float l, int Kt, int& over) {
    if (!(l >= 0.f)) return -2;
    if (l != floorf(l)) return -1;
    if (l >= (float)Kt) {
        over = 1;
        return -1;
    }
    return (int)l;
}

// 64 channels x 64 lanes -> lane j gets channel j summed over the lanes: a butterfly that halves the channels a lane keeps at every
// step (63 exchanges for 64 channels, where a wave_sum per channel takes 6 each).  Lane bit o set keeps channel c + o, clear keeps c,
// so the channel a lane ends with is its own number.  v_permlane32_swap / v_permlane16_swap exchange the halves of a register pair
// in one instruction; the four steps inside a 16-lane row are DPP.  A fixed association: the same bits on every call.
__device__ __forceinline__ float reduce_scatter64(float (&v)[64], int lane) {
    typedef unsigned u32x2s __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const u32x2s r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[i]), __float_as_uint(v[i + 32]), false, false);
        v[i] = __uint_as_float(r.x) + __uint_as_float(r.y);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const u32x2s r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[i]), __float_as_uint(v[i + 16]), false, false);
        v[i] = __uint_as_float(r.x) + __uint_as_float(r.y);
    }
    const bool b8 = lane & 8, b4 = lane & 4, b2 = lane & 2, b1 = lane & 1;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (b8 ? v[i + 8] : v[i]) + msm::wave_xor_dpp8(b8 ? v[i] : v[i + 8]);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (b4 ? v[i + 4] : v[i]) + msm::wave_xor_dpp4(b4 ? v[i] : v[i + 4]);
#pragma unroll
    for (int i = 0; i < 2; ++i) v[i] = (b2 ? v[i + 2] : v[i]) + msm::wave_xor_dpp2(b2 ? v[i] : v[i + 2]);
    return (b1 ? v[1] : v[0]) + msm::wave_xor_dpp1(b1 ? v[0] : v[1]);
}

// v[j] = x[cb + j][p], 0 for cb + j >= C: 64 coalesced loads in flight per wave, each a uniform row base plus the lane's pixel
// (every lane loads -- its pixel is in bounds -- and the caller masks; a load per lane under a condition would be a branch each)
__device__ __forceinline__ void load_chunk(float (&v)[64], const float* xb, unsigned p, int cb, int C, int64_t HW) {
    const float* row = xb + (int64_t)cb * HW;
    if (cb + 64 <= C) {
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            v[j] = (row + (int64_t)j * HW)[p];
            if ((j & 15) == 15) __builtin_amdgcn_sched_barrier(0);      // loads stay in groups of 16 (the row bases are scalar registers)
        }
    } else {
#pragma unroll
        for (int j = 0; j < 64; ++j) v[j] = cb + j < C ? (row + (int64_t)j * HW)[p] : 0.f;
    }
}

__device__ __forceinline__ int wave_max_int(int v) {
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max_float(float v) {
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// the waves' private tables added in wave order, rows 0 .. kmax, into the workgroup's partial
template <int W>
__device__ __forceinline__ void write_partial(const float* lds, float* part, int stride, int Kt, int C, int kmax, int tid, bool with_rows) {
    const int rows = with_rows ? (kmax + 1) * C : 0;
    for (int i = tid; i < rows; i += 64 * W) {
        float s = lds[i];
        for (int w = 1; w < W; ++w) s += lds[w * stride + i];
        part[i] = s;
    }
    for (int k = tid; k <= kmax; k += 64 * W) {
        int n = 0;
        float d = 0.f;
        for (int w = 0; w < W; ++w) {
            n += ((const int*)lds)[w * stride + Kt * C + k];
            d += lds[w * stride + Kt * C + Kt + k];
        }
        ((int*)part)[Kt * C + k] = n;
        part[Kt * C + Kt + k] = d;
    }
}

template <int W>
__global__ __launch_bounds__(64 * W) void embloss_stats_kernel(const float* __restrict__ x, const float* __restrict__ lab,
                                                                float* __restrict__ part, int* __restrict__ wginfo, int C, int HW,
                                                                int Kt, int chunk, int pstride) {
    extern __shared__ float lds[];
    __shared__ int s_k[W], s_o[W];
    __shared__ float s_l[W];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = blockIdx.x, b = blockIdx.y, G = gridDim.x;
    const int stride = Kt * C + 2 * Kt;
    float* T = lds + wave * stride;
    int* Cn = (int*)(T + Kt * C);
    for (int i = tid; i < W * stride; i += 64 * W) lds[i] = 0.f;
    __syncthreads();
    const int p0 = g * chunk, p1 = min(HW, p0 + chunk);
    const float* xb = x + (int64_t)b * C * HW;
    int kmax = -1, over = 0;
    float lmax = -1.f;
    for (int base = p0 + wave * 64; base < p1; base += 64 * W) {
        const int p = base + lane;
        const bool valid = p < p1;
        const int pc = valid ? p : p1 - 1;
        const float l = valid ? lab[(int64_t)b * HW + pc] : -1.f;
        const int k = cluster_of(l, Kt, over);
        kmax = max(kmax, k);
        lmax = fmaxf(lmax, l);
        unsigned long long rem = __ballot(k >= 0);
        while (rem) {
            const int k0 = __builtin_amdgcn_readfirstlane(__shfl(k, __ffsll((long long)rem) - 1));
            const bool mine = k == k0;
            const unsigned long long m = __ballot(mine);
            rem &= ~m;
            if (lane == 0) Cn[k0] += __popcll(m);
            for (int cb = 0; cb < C; cb += 64) {
                float v[64];
                load_chunk(v, xb, pc, cb, C, HW);
#pragma unroll
                for (int j = 0; j < 64; ++j) v[j] = mine ? v[j] : 0.f;
                const float r = reduce_scatter64(v, lane);
                if (cb + lane < C) T[k0 * C + cb + lane] += r;
            }
        }
    }
    kmax = wave_max_int(kmax), over = wave_max_int(over), lmax = wave_max_float(lmax);
    if (lane == 0) s_k[wave] = kmax, s_o[wave] = over, s_l[wave] = lmax;
    __syncthreads();
    for (int w = 0; w < W; ++w) kmax = max(kmax, s_k[w]), over = max(over, s_o[w]), lmax = fmaxf(lmax, s_l[w]);
    const int64_t wg = (int64_t)b * G + g;
    write_partial<W>(lds, part + wg * pstride, stride, Kt, C, kmax, tid, true);
    if (tid == 0) {
        wginfo[wg * 4 + 0] = kmax;
        wginfo[wg * 4 + 1] = __float_as_int(lmax);
        wginfo[wg * 4 + 2] = over;
        wginfo[wg * 4 + 3] = 0;
    }
}

// sum of v over the 256 threads in a fixed tree; every thread gets it
__device__ __forceinline__ float block_sum256(float v, float* s4, int tid) {
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) s4[tid >> 6] = v;
    __syncthreads();
    return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// The workgroups' partials of image b summed in workgroup order: 16 table entries per block, each by 16 threads that take a
// sixteenth of the workgroups in order and are then added in that order (a short dependent chain per thread: a partial is read
// only after its workgroup's row count).  A workgroup wrote rows 0 .. its own largest cluster
// only, so the others are skipped (never read).  rows -> rows_out [B][Kt C] (when given), counts -> cnt_out [B][Kt] int, the d^2
// sums -> D_out [B][Kt] (when given); one more block sums the strays' d^2 and hard counts -> stray_out [B][2] (when given).
__global__ __launch_bounds__(256) void embloss_sum_kernel(const float* __restrict__ part, const int* __restrict__ wginfo,
                                                           float* __restrict__ rows_out, int* __restrict__ cnt_out, float* __restrict__ D_out,
                                                           float* __restrict__ stray_out, int C, int Kt, int G, int pstride) {
    __shared__ float s_f[16][16];
    __shared__ int s_i[16][16];
    const int tid = threadIdx.x, b = blockIdx.y;
    if (stray_out && blockIdx.x == gridDim.x - 1) {
        float s = 0.f;
        int h = 0;
        for (int g = tid; g < G; g += 256) {
            const float* pw = part + ((int64_t)b * G + g) * pstride;
            s += pw[Kt * C + 2 * Kt];
            h += ((const int*)pw)[Kt * C + 2 * Kt + 1];
        }
        s = block_sum256(s, &s_f[0][0], tid);
        for (int o = 32; o; o >>= 1) h += __shfl_xor(h, o);
        if ((tid & 63) == 0) s_i[0][tid >> 6] = h;
        __syncthreads();
        if (tid == 0) {
            stray_out[b * 2] = s;
            ((int*)stray_out)[b * 2 + 1] = s_i[0][0] + s_i[0][1] + s_i[0][2] + s_i[0][3];
        }
        return;
    }
    const int i = tid & 15, q = tid >> 4;
    const int first = rows_out ? 0 : Kt * C, last = Kt * C + (D_out ? 2 * Kt : Kt);
    const int idx = first + blockIdx.x * 16 + i;
    const bool valid = idx < last, is_int = idx >= Kt * C && idx < Kt * C + Kt;
    const int k = idx < Kt * C ? idx / C : (idx - Kt * C) % Kt;
    const int Gq = (G + 15) / 16, g1 = min(G, (q + 1) * Gq);
    float s = 0.f;
    int si = 0;
    if (valid)
        for (int g = q * Gq; g < g1; ++g) {
            const int64_t wg = (int64_t)b * G + g;
            if (wginfo[wg * 4] >= k) {
                if (is_int) si += ((const int*)part)[wg * pstride + idx];
                else s += part[wg * pstride + idx];
            }
        }
    s_f[q][i] = s, s_i[q][i] = si;
    __syncthreads();
    if (q == 0 && valid) {
        float tf = s_f[0][i];
        int ti = s_i[0][i];
        for (int r = 1; r < 16; ++r) tf += s_f[r][i], ti += s_i[r][i];
        if (idx < Kt * C) rows_out[(int64_t)b * Kt * C + idx] = tf;
        else if (is_int) cnt_out[b * Kt + idx - Kt * C] = ti;
        else D_out[b * Kt + idx - Kt * C - Kt] = tf;
    }
}

__global__ __launch_bounds__(256) void embloss_finish_kernel(const int* __restrict__ wginfo, int* __restrict__ info,
                                                              const float* __restrict__ S, float* __restrict__ mu,
                                                              float* __restrict__ nrm, float* __restrict__ H, float* __restrict__ irow,
                                                              float* __restrict__ GI, int B, int C, int Kt, int G, int metric,
                                                              int normalize, float delta) {
    __shared__ float s_l[4];
    __shared__ int s_o[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    float lmax = -1.f;
    int over = 0;
    for (int i = tid; i < B * G; i += 256) {
        lmax = fmaxf(lmax, __int_as_float(wginfo[(int64_t)i * 4 + 1]));
        over = max(over, wginfo[(int64_t)i * 4 + 2]);
    }
    lmax = wave_max_float(lmax), over = wave_max_int(over);
    if (lane == 0) s_l[wave] = lmax, s_o[wave] = over;
    __syncthreads();
    lmax = fmaxf(fmaxf(s_l[0], s_l[1]), fmaxf(s_l[2], s_l[3]));
    over = max(max(s_o[0], s_o[1]), max(s_o[2], s_o[3]));
    const int K = lmax >= 0.f ? (int)fminf(lmax, 1.0e9f) + 1 : 1;       // no labelled pixel at all: K = 1, every term 0
    const int Ka = min(K, Kt);
    if (b == 0 && tid == 0) info[0] = K, info[1] = over, info[3] = 0;
    const int* n_out = info + EL_INFO_HDR + b * Kt;
    const float* Sb = S + (int64_t)b * Kt * C;
    float* mub = mu + (int64_t)b * Kt * C;
    float* GIb = GI + (int64_t)b * Kt * C;
    float* Hb = H + (int64_t)b * Kt * Kt;
    for (int k = wave; k < Ka; k += 4) {
        const float den = (float)n_out[k] + 1e-10f;
        float ss = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float m = Sb[k * C + c] / den;
            ss += m * m;
        }
        const float nr = sqrtf(wave_sum(ss));
        const float r = normalize ? fmaxf(nr, 1e-12f) : 1.f;
        for (int c = lane; c < C; c += 64) mub[k * C + c] = (Sb[k * C + c] / den) / r;
        if (lane == 0) nrm[b * Kt + k] = nr;
    }
    __syncthreads();
    for (int i = wave; i < Ka; i += 4) {
        float rowsum = 0.f;
        for (int j = 0; j < Ka; ++j) {
            float acc = 0.f;
            for (int c = lane; c < C; c += 64) {
                const float a = mub[i * C + c], q = mub[j * C + c];
                acc += metric == 0 ? a * q : (a - q) * (a - q);
            }
            acc = wave_sum(acc);
            const float dist = metric == 0 ? 0.5f * (1.f - acc) : sqrtf(acc);
            const float h = (i != j && K > 1) ? fmaxf(delta - dist, 0.f) : 0.f;
            rowsum += h * h;
            // d/d mu_i of the sum over ORDERED pairs (every pair twice): cosine 2 h mu_j, euclidean -4 h (mu_i - mu_j) / dist
            if (lane == 0) Hb[i * Kt + j] = metric == 0 ? 2.f * h : (dist > 0.f ? -4.f * h / dist : 0.f);
        }
        if (lane == 0) irow[b * Kt + i] = rowsum;
    }
    for (int i = Ka + tid; i < Kt; i += 256) irow[b * Kt + i] = 0.f;
    __syncthreads();
    for (int idx = tid; idx < Ka * C; idx += 256) {
        const int i = idx / C, c = idx - i * C;
        const float a = mub[idx];
        float acc = 0.f;
        for (int j = 0; j < Ka; ++j) {
            const float coef = Hb[i * Kt + j];
            acc += metric == 0 ? coef * mub[j * C + c] : coef * (a - mub[j * C + c]);
        }
        GIb[idx] = acc;
    }
}

template <int W, int METRIC>
__global__ __launch_bounds__(64 * W) void embloss_dist_kernel(const float* __restrict__ x, const float* __restrict__ lab,
                                                               const float* __restrict__ mu, const int* __restrict__ wginfo,
                                                               float* __restrict__ part, int C, int HW, int Kt, int chunk, int pstride,
                                                               float alpha) {
    extern __shared__ float lds[];
    __shared__ float s_s[W];
    __shared__ int s_h[W];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = blockIdx.x, b = blockIdx.y, G = gridDim.x;
    const int stride = Kt * C + 2 * Kt;
    float* T = lds + wave * stride;
    int* Nw = (int*)(T + Kt * C);
    float* Dw = T + Kt * C + Kt;
    for (int i = tid; i < W * stride; i += 64 * W) lds[i] = 0.f;
    __syncthreads();
    const int p0 = g * chunk, p1 = min(HW, p0 + chunk);
    const float* xb = x + (int64_t)b * C * HW;
    const float* mub = mu + (int64_t)b * Kt * C;
    float stray = 0.f;
    int stray_hard = 0, over = 0;                          // `over` was recorded by the stats pass
    for (int base = p0 + wave * 64; base < p1; base += 64 * W) {
        const int p = base + lane;
        const bool valid = p < p1;
        const int pc = valid ? p : p1 - 1;
        const float l = valid ? lab[(int64_t)b * HW + pc] : -1.f;
        const int k = cluster_of(l, Kt, over);
        const float* xp = xb + pc;
        unsigned long long rem = __ballot(k >= 0);
        while (rem) {
            const int k0 = __builtin_amdgcn_readfirstlane(__shfl(k, __ffsll((long long)rem) - 1));
            const bool mine = k == k0;
            rem &= ~__ballot(mine);
            const float* mk = mub + k0 * C;
            float v[64];
            float acc = 0.f;
            for (int cb = 0; cb < C; cb += 64) {
                load_chunk(v, xb, pc, cb, C, HW);
#pragma unroll
                for (int j = 0; j < 64; ++j) {
                    const float q = cb + j < C ? mk[cb + j] : 0.f;
                    acc += METRIC == 0 ? v[j] * q : (v[j] - q) * (v[j] - q);
                    if ((j & 15) == 15) __builtin_amdgcn_sched_barrier(0);      // 16 centre values live at a time
                }
            }
            const float d = METRIC == 0 ? 0.5f * (1.f - acc) : sqrtf(acc);
            const float dsum = wave_sum(mine ? d * d : 0.f);
            const int hard = __popcll(__ballot(mine && d > alpha));
            if (lane == 0) Dw[k0] += dsum, Nw[k0] += hard;
            if (METRIC == 0)                                // T += d_p x_p; up to 64 channels are still in registers
                for (int cb = 0; cb < C; cb += 64) {
                    if (C > 64) load_chunk(v, xb, pc, cb, C, HW);
#pragma unroll
                    for (int j = 0; j < 64; ++j) v[j] = mine ? v[j] * d : 0.f;
                    const float r = reduce_scatter64(v, lane);
                    if (cb + lane < C) T[k0 * C + cb + lane] += r;
                }
        }
        if (__ballot(k == -1)) {                            // labelled pixels of no cluster: the centre is 0
            const bool mine = k == -1;
            float d = 0.5f;
            if (METRIC != 0) {
                float acc = 0.f;
#pragma unroll 8
                for (int c = 0; c < C; ++c) {
                    const float v = mine ? xp[(int64_t)c * HW] : 0.f;
                    acc += v * v;
                }
                d = sqrtf(acc);
            }
            stray += wave_sum(mine ? d * d : 0.f);
            stray_hard += __popcll(__ballot(mine && d > alpha));
        }
    }
    if (lane == 0) s_s[wave] = stray, s_h[wave] = stray_hard;
    __syncthreads();
    const int64_t wg = (int64_t)b * G + g;
    float* pw = part + wg * pstride;
    write_partial<W>(lds, pw, stride, Kt, C, wginfo[wg * 4], tid, METRIC == 0);
    if (tid == 0) {
        float s = 0.f;
        int h = 0;
        for (int w = 0; w < W; ++w) s += s_s[w], h += s_h[w];
        pw[Kt * C + 2 * Kt] = s;
        ((int*)pw)[Kt * C + 2 * Kt + 1] = h;
    }
}

__global__ __launch_bounds__(256) void embloss_finalize_kernel(int* __restrict__ info, float* __restrict__ hdr, const float* __restrict__ S,
                                                                const float* __restrict__ mu, const float* __restrict__ nrm,
                                                                const float* __restrict__ T, const float* __restrict__ D,
                                                                const float* __restrict__ stray, const float* __restrict__ irow,
                                                                float* __restrict__ coef, float* __restrict__ VI, float* __restrict__ VE,
                                                                float* __restrict__ losses, int B, int C, int Kt, int metric, int normalize,
                                                                float lambda_intra, float lambda_inter) {
    __shared__ float s4[4];
    __shared__ int s_h[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int K = info[0], Ka = min(K, Kt);
    const int* n_all = info + EL_INFO_HDR;
    const int* N_all = info + EL_INFO_HDR + B * Kt;
    int hard = 0;                                           // the reference's torch.sum(intra_cluster_mask): every labelled pixel counts
    for (int i = tid; i < B * Kt; i += 256) hard |= N_all[i];
    for (int i = tid; i < B; i += 256) hard |= ((const int*)stray)[i * 2 + 1];
    hard = wave_max_int(hard);
    if (lane == 0) s_h[wave] = hard;
    __syncthreads();
    const bool flag = (s_h[0] | s_h[1] | s_h[2] | s_h[3]) != 0;
    const float cI = flag ? lambda_intra / (float)B : 0.f;
    const float a_s = cI / (50.f * (float)K);
    const float c_inter = K > 1 ? lambda_inter / (0.5f * (float)K * (float)(K - 1) * (float)B) : 0.f;
    for (int k = tid; k < Kt; k += 256) coef[b * Kt + k] = cI / ((float)K * fmaxf((float)N_all[b * Kt + k], 50.f));
    if (b == 0) {
        float vi = 0.f, ve = 0.f;
        for (int i = tid; i < B * Kt; i += 256) {
            vi += D[i] * (cI / ((float)K * fmaxf((float)N_all[i], 50.f)));
            ve += irow[i];
        }
        for (int i = tid; i < B; i += 256) vi += stray[i * 2] * a_s;
        vi = block_sum256(vi, s4, tid);
        ve = block_sum256(ve, s4, tid) * c_inter;
        if (tid == 0) {
            losses[0] = vi + ve, losses[1] = vi, losses[2] = ve;
            info[2] = flag ? 1 : 0;
            hdr[0] = a_s;
        }
    }
    // the gradient with respect to each centre, taken back through the normalisation and spread over the cluster's n pixels
    for (int k = wave; k < Ka; k += 4) {
        const int64_t row = ((int64_t)b * Kt + k) * C;
        const int n = n_all[b * Kt + k];
        if (n == 0) {                                       // nothing is propagated into an empty cluster
            for (int c = lane; c < C; c += 64) VI[row + c] = 0.f, VE[row + c] = 0.f;
            continue;
        }
        const float a = cI / ((float)K * fmaxf((float)N_all[b * Kt + k], 50.f));
        const float nf = (float)n, inv_n = 1.f / (nf + 1e-10f);
        const float nr = nrm[b * Kt + k];
        const bool through = normalize && nr > 1e-12f;
        const float r = normalize ? fmaxf(nr, 1e-12f) : 1.f;
        float pI = 0.f, pE = 0.f;
        if (through) {
            for (int c = lane; c < C; c += 64) {
                const float m = mu[row + c];
                const float gI = metric == 0 ? -a * T[row + c] : -2.f * a * (S[row + c] - nf * m);
                pI += gI * m;
                pE += c_inter * VE[row + c] * m;
            }
            pI = wave_sum(pI), pE = wave_sum(pE);
        }
        for (int c = lane; c < C; c += 64) {
            const float m = mu[row + c];
            const float gI = metric == 0 ? -a * T[row + c] : -2.f * a * (S[row + c] - nf * m);
            const float gE = c_inter * VE[row + c];
            VI[row + c] = (gI - m * pI) / r * inv_n;
            VE[row + c] = (gE - m * pE) / r * inv_n;
        }
    }
}

template <int METRIC>
__global__ __launch_bounds__(256) void embloss_bwd_kernel(const float* __restrict__ x, const float* __restrict__ lab,
                                                           const float* __restrict__ gl, const float* __restrict__ hdr,
                                                           const float* __restrict__ mu, const float* __restrict__ coef,
                                                           const float* __restrict__ VI, const float* __restrict__ VE,
                                                           float* __restrict__ gx, int C, int HW, int Kt) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const float gi = gl[0] + gl[1], ge = gl[0] + gl[2];
    int over = 0;
    const int k = cluster_of(lab[(int64_t)b * HW + p], Kt, over);
    const float* xp = x + (int64_t)b * C * HW + p;
    float* gp = gx + (int64_t)b * C * HW + p;
    if (k == -2 || (k == -1 && METRIC == 0)) {
        for (int c = 0; c < C; ++c) gp[(int64_t)c * HW] = 0.f;
    } else if (k == -1) {
        const float w = 2.f * gi * hdr[0];
#pragma unroll 4
        for (int c = 0; c < C; ++c) gp[(int64_t)c * HW] = w * xp[(int64_t)c * HW];
    } else {
        const int64_t row = ((int64_t)b * Kt + k) * C;
        const float a = coef[b * Kt + k];
        if (METRIC == 0) {
            float dot = 0.f;
#pragma unroll 8
            for (int c = 0; c < C; ++c) dot += xp[(int64_t)c * HW] * mu[row + c];
            const float w = -gi * a * (0.5f * (1.f - dot));
#pragma unroll 4
            for (int c = 0; c < C; ++c) gp[(int64_t)c * HW] = w * mu[row + c] + (gi * VI[row + c] + ge * VE[row + c]);
        } else {
            const float w = 2.f * gi * a;
#pragma unroll 4
            for (int c = 0; c < C; ++c)
                gp[(int64_t)c * HW] = w * (xp[(int64_t)c * HW] - mu[row + c]) + (gi * VI[row + c] + ge * VE[row + c]);
        }
    }
}

template <int W>
int launch_passes(const Plan& P, const float* x, const float* lab, float* ws, int B, int C, int HW, int Kt, int metric,
                  float alpha, int which, hipStream_t s) {
    const size_t lds = (size_t)W * (Kt * C + 2 * Kt) * sizeof(float);
    float* part = ws + P.o_part;
    int* wginfo = (int*)(ws + P.o_wginfo);
    if (which == 0) {
        MSM_CHECK_HIP((hipError_t)msm::ensure_dynamic_lds((const void*)embloss_stats_kernel<W>, lds));
        hipLaunchKernelGGL(embloss_stats_kernel<W>, dim3(P.G, B), dim3(64 * W), lds, s, x, lab, part, wginfo, C, HW, Kt, P.chunk, P.pstride);
    } else if (metric == 0) {
        MSM_CHECK_HIP((hipError_t)msm::ensure_dynamic_lds((const void*)embloss_dist_kernel<W, 0>, lds));
        hipLaunchKernelGGL((embloss_dist_kernel<W, 0>), dim3(P.G, B), dim3(64 * W), lds, s, x, lab, ws + P.o_mu, wginfo, part, C, HW, Kt,
                           P.chunk, P.pstride, alpha);
    } else {
        MSM_CHECK_HIP((hipError_t)msm::ensure_dynamic_lds((const void*)embloss_dist_kernel<W, 1>, lds));
        hipLaunchKernelGGL((embloss_dist_kernel<W, 1>), dim3(P.G, B), dim3(64 * W), lds, s, x, lab, ws + P.o_mu, wginfo, part, C, HW, Kt,
                           P.chunk, P.pstride, alpha);
    }
    MSM_CHECK_LAUNCH(which == 0 ? "msm_embloss_fwd (stats)" : "msm_embloss_fwd (distances)");
    return MSM_OK;
}

int launch_pass(const Plan& P, const float* x, const float* lab, float* ws, int B, int C, int HW, int Kt, int metric,
                float alpha, int which, hipStream_t s) {
    if (P.W == 4) return launch_passes<4>(P, x, lab, ws, B, C, HW, Kt, metric, alpha, which, s);
    if (P.W == 2) return launch_passes<2>(P, x, lab, ws, B, C, HW, Kt, metric, alpha, which, s);
    return launch_passes<1>(P, x, lab, ws, B, C, HW, Kt, metric, alpha, which, s);
}

const char* const SHAPE_MSG = "%s: B=%d C=%d HW=%d max_clusters=%d outside 0 < B <= 65535, C >= 1, HW >= 1, 1 <= max_clusters <= 1024, max_clusters * C <= 16384";

}  // namespace

extern "C" int64_t msm_embloss_workspace(int B, int C, int HW, int max_clusters) {
    if (!shape_ok(B, C, HW, max_clusters)) {
        msm::set_error(SHAPE_MSG, "msm_embloss_workspace", B, C, HW, max_clusters);
        return MSM_E_INVALID;
    }
    return plan(B, C, HW, max_clusters).total * 4;
}

extern "C" int msm_embloss_fwd(const float* x, const float* labels, float* losses, int32_t* info, void* workspace, int64_t workspace_bytes,
                               int B, int C, int HW, int max_clusters, int metric, int normalize, float alpha, float delta,
                               float lambda_intra, float lambda_inter, void* stream) {
    const int Kt = max_clusters;
    MSM_REQUIRE(shape_ok(B, C, HW, Kt), SHAPE_MSG, "msm_embloss_fwd", B, C, HW, Kt);
    MSM_REQUIRE(metric == 0 || metric == 1, "msm_embloss_fwd: metric %d is neither 0 (cosine) nor 1 (euclidean)", metric);
    MSM_REQUIRE(x && labels && losses && info && workspace, "msm_embloss_fwd: null pointer");
    const Plan P = plan(B, C, HW, Kt);
    if (workspace_bytes < P.total * 4) {
        msm::set_error("msm_embloss_fwd: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)P.total * 4);
        return MSM_E_WORKSPACE;
    }
    float* ws = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    int rc = launch_pass(P, x, labels, ws, B, C, HW, Kt, metric, alpha, 0, s);
    if (rc != MSM_OK) return rc;
    const float* part = ws + P.o_part;
    const int* wginfo = (const int*)(ws + P.o_wginfo);
    int32_t* n_out = info + EL_INFO_HDR;
    hipLaunchKernelGGL(embloss_sum_kernel, dim3(msm::cdiv((int64_t)Kt * C + Kt, 16), B), dim3(256), 0, s, part, wginfo, ws + P.o_S, n_out,
                       (float*)nullptr, (float*)nullptr, C, Kt, P.G, P.pstride);
    MSM_CHECK_LAUNCH("msm_embloss_fwd (sum of the statistics)");
    hipLaunchKernelGGL(embloss_finish_kernel, dim3(B), dim3(256), 0, s, wginfo, info, ws + P.o_S, ws + P.o_mu, ws + P.o_nrm, ws + P.o_H,
                       ws + P.o_irow, ws + P.o_VE, B, C, Kt, P.G, metric, normalize, delta);
    MSM_CHECK_LAUNCH("msm_embloss_fwd (finish)");
    rc = launch_pass(P, x, labels, ws, B, C, HW, Kt, metric, alpha, 1, s);
    if (rc != MSM_OK) return rc;
    // cosine: T rows, N, D; euclidean: N and D only (its centre path follows from S, n and mu); + 1 block for the strays
    hipLaunchKernelGGL(embloss_sum_kernel, dim3(msm::cdiv((metric == 0 ? (int64_t)Kt * C : 0) + 2 * Kt, 16) + 1, B), dim3(256), 0, s, part,
                       wginfo, metric == 0 ? ws + P.o_T : (float*)nullptr, n_out + (int64_t)B * Kt, ws + P.o_D, ws + P.o_stray, C, Kt, P.G,
                       P.pstride);
    MSM_CHECK_LAUNCH("msm_embloss_fwd (sum of the distances)");
    hipLaunchKernelGGL(embloss_finalize_kernel, dim3(B), dim3(256), 0, s, info, ws, ws + P.o_S, ws + P.o_mu, ws + P.o_nrm, ws + P.o_T,
                       ws + P.o_D, ws + P.o_stray, ws + P.o_irow, ws + P.o_coef, ws + P.o_VI, ws + P.o_VE, losses, B, C, Kt, metric,
                       normalize, lambda_intra, lambda_inter);
    MSM_CHECK_LAUNCH("msm_embloss_fwd (finalize)");
    return MSM_OK;
}

extern "C" int msm_embloss_bwd(const float* x, const float* labels, const float* grad_losses, const void* workspace,
                               int64_t workspace_bytes, float* grad_x, int B, int C, int HW, int max_clusters, int metric, void* stream) {
    const int Kt = max_clusters;
    MSM_REQUIRE(shape_ok(B, C, HW, Kt), SHAPE_MSG, "msm_embloss_bwd", B, C, HW, Kt);
    MSM_REQUIRE(metric == 0 || metric == 1, "msm_embloss_bwd: metric %d is neither 0 (cosine) nor 1 (euclidean)", metric);
    MSM_REQUIRE(x && labels && grad_losses && workspace && grad_x, "msm_embloss_bwd: null pointer");
    const Plan P = plan(B, C, HW, Kt);
    if (workspace_bytes < P.total * 4) {
        msm::set_error("msm_embloss_bwd: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)P.total * 4);
        return MSM_E_WORKSPACE;
    }
    const float* ws = (const float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(msm::cdiv(HW, 256), B);
    if (metric == 0)
        hipLaunchKernelGGL(embloss_bwd_kernel<0>, grid, dim3(256), 0, s, x, labels, grad_losses, ws, ws + P.o_mu, ws + P.o_coef, ws + P.o_VI,
                           ws + P.o_VE, grad_x, C, HW, Kt);
    else
        hipLaunchKernelGGL(embloss_bwd_kernel<1>, grid, dim3(256), 0, s, x, labels, grad_losses, ws, ws + P.o_mu, ws + P.o_coef, ws + P.o_VI,
                           ws + P.o_VE, grad_x, C, HW, Kt);
    MSM_CHECK_LAUNCH("msm_embloss_bwd");
    return MSM_OK;
}
