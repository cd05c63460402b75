// The Mask2Former set criterion of the reference (MSMFormer/meanshiftformer/modeling/matcher.py, criterion.py) on point-sampled
// masks, for every prediction of one criterion call (the final one and the auxiliary ones) at once.
//
// point_sample(x, c) = grid_sample(x, 2c - 1, bilinear, zeros, align_corners=False): ix = c_x W - 0.5, iy = c_y H - 0.5, four
// taps in torch's order (nw, ne, sw, se), taps outside the map read 0.  c[..., 0] is x (the width axis).
//
//   match_cost_kernel       C[q][t] = w_mask cost_mask + w_class cost_class + w_dice cost_dice for every (prediction, image):
//                           one workgroup per 16 x 16 (query, target) tile; each wave takes every fourth chunk of 4 points,
//                           samples x (a query's logits) as the A operand and y (a target's labels) as the B operand of
//                           v_mfma_f32_16x16x4_f32 and contracts x.y and sigma(x).y; softplus(-x) = softplus(x) - x turns the
//                           sigmoid-CE cost into row sums plus the x.y contraction.  No Q x P plane is stored.
//   point_loss_fwd_kernel   one workgroup per matched (prediction, mask): exact top-k of the uncertainty -|x| over the
//                           oversampled points (radix select on the |x| bits, ties to the lower index), then the sigmoid-CE and
//                           dice terms over the k selected + P - k uniform points; writes the selection (bitmap and the index
//                           list the backward reads) and the per-mask terms.
//   point_loss_sum_kernel   one wave per prediction sums its per-mask terms in a fixed order (bit-reproducible losses).
//   point_loss_bwd_kernel   one workgroup per matched mask: dL/dx per point, scattered through the four bilinear weights into
//                           an LDS copy of the mask (written out whole): 64-bit fixed point and integer atomics where the mask
//                           fits (bit-reproducible gradients), floats above that, or, for large masks, global float atomics.
#include "common.h"

namespace {

using namespace msm;

constexpr int CR_THREADS = 256;
constexpr int CR_WAVES = CR_THREADS / 64;
constexpr int64_t CR_LDS_MAX = 128 * 1024;     // bytes of one mask's gradient accumulated in LDS as floats
constexpr int64_t CR_LDS_FIX_MAX = 160 * 1024; // ... and as 64-bit fixed point (the whole LDS of a CU: one workgroup on it)

// grid_sample's source coordinate for align_corners=False, from the point_sample grid 2c - 1 (clamped so that a stray value
// can never produce an out-of-range tap index; every in-range value is unchanged)
__device__ __forceinline__ float cr_src(float c, int size) {
    const float g = 2.f * c - 1.f;
    const float i = ((g + 1.f) * (float)size - 1.f) * 0.5f;
    return fminf(fmaxf(i, -2.f), (float)size + 1.f);
}

__device__ __forceinline__ float cr_load(const float* p, int i) { return p[i]; }
__device__ __forceinline__ float cr_load(const uint8_t* p, int i) { return (float)p[i]; }

template <typename T>
__device__ __forceinline__ float cr_sample(const T* __restrict__ m, int H, int W, float cx, float cy) {
    const float ix = cr_src(cx, W), iy = cr_src(cy, H);
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float e = ix - fx, w = (fx + 1.f) - ix, s = iy - fy, n = (fy + 1.f) - iy;
    const bool xa = x0 >= 0 && x0 < W, xb = x0 + 1 >= 0 && x0 + 1 < W;
    float v = 0.f;
    if (y0 >= 0 && y0 < H) {
        if (xa) v += w * n * cr_load(m, y0 * W + x0);
        if (xb) v += e * n * cr_load(m, y0 * W + x0 + 1);
    }
    if (y0 + 1 >= 0 && y0 + 1 < H) {
        if (xa) v += w * s * cr_load(m, (y0 + 1) * W + x0);
        if (xb) v += e * s * cr_load(m, (y0 + 1) * W + x0 + 1);
    }
    return v;
}

__device__ __forceinline__ float cr_sigmoid(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float cr_softplus(float x) { return fmaxf(x, 0.f) + log1pf(__expf(-fabsf(x))); }

// ---------------------------------------------------------------------------------------------------------------------------
// (a) matching costs.  table: [n_pred] logits pointers, [n_pred] mask pointers, [B + 1] target offsets (int64 each).
__global__ __launch_bounds__(CR_THREADS) void match_cost_kernel(const int64_t* __restrict__ table, const uint8_t* __restrict__ tgt,
                                                                const int32_t* __restrict__ labels, const float* __restrict__ pts,
                                                                float* __restrict__ cost, int n_pred, int B, int Q, int C1, int Hm,
                                                                int Wm, int Hg, int Wg, int P, int TT, float wc, float wm, float wd) {
    __shared__ float red[CR_WAVES][11][64];
    __shared__ float rows[3][16];
    const int pred = blockIdx.z / B, b = blockIdx.z % B;
    const int t_begin = (int)table[2 * n_pred + b];
    const int T = (int)table[2 * n_pred + b + 1] - t_begin;
    const int t0 = blockIdx.y * 16, q0 = blockIdx.x * 16;
    if (t0 >= T || t_begin < 0 || t_begin + T > TT) return;                               // uniform over the workgroup
    const float* logits = reinterpret_cast<const float*>(table[pred]) + (size_t)b * Q * C1;
    const float* masks = reinterpret_cast<const float*>(table[n_pred + pred]) + (size_t)b * Q * Hm * Wm;
    const float* pt = pts + ((size_t)pred * B + b) * P * 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i16 = lane & 15, kk = lane >> 4;
    const bool qok = q0 + i16 < Q, tok = t0 + i16 < T;
    const float* mq = masks + (size_t)(qok ? q0 + i16 : 0) * Hm * Wm;
    const uint8_t* mt = tgt + (size_t)(t_begin + (tok ? t0 + i16 : 0)) * Hg * Wg;

    f32x4 dxy = {0.f, 0.f, 0.f, 0.f}, dsy = {0.f, 0.f, 0.f, 0.f};
    float sp = 0.f, sg = 0.f, ys = 0.f;
    const int nchunk = (P + 3) >> 2;
    for (int c = wave; c < nchunk; c += CR_WAVES) {                                       // wave-uniform trip count
        const int p = 4 * c + kk;
        float x = 0.f, s = 0.f, y = 0.f;
        if (p < P) {
            const float cx = pt[2 * p], cy = pt[2 * p + 1];
            if (qok) {
                x = cr_sample(mq, Hm, Wm, cx, cy);
                s = cr_sigmoid(x);
                sp += cr_softplus(x);
                sg += s;
            }
            if (tok) {
                y = cr_sample(mt, Hg, Wg, cx, cy);
                ys += y;
            }
        }
        dxy = mfma16(x, y, dxy);                       // A[q][p] = x, B[p][t] = y
        dsy = mfma16(s, y, dsy);
    }
    for (int r = 0; r < 4; ++r) {
        red[wave][r][lane] = dxy[r];
        red[wave][4 + r][lane] = dsy[r];
    }
    red[wave][8][lane] = sp;
    red[wave][9][lane] = sg;
    red[wave][10][lane] = ys;
    __syncthreads();
    float v[11];                                       // every wave sums the four partials in the same order; wave 0 finishes
    for (int j = 0; j < 11; ++j) {
        float a = red[0][j][lane];
        for (int w = 1; w < CR_WAVES; ++w) a += red[w][j][lane];
        v[j] = a;
    }
    // row sums: lane (i16, kk) holds the partial of row / column i16 over its point slot kk
    const float rsp = sum_lane_rows(v[8]), rsg = sum_lane_rows(v[9]), rys = sum_lane_rows(v[10]);
    if (wave == 0 && lane < 16) {
        rows[0][lane] = rsp;
        rows[1][lane] = rsg;
        rows[2][lane] = rys;
    }
    __syncthreads();
    if (wave != 0) return;
    const int t = t0 + i16;
    if (t >= T) return;
    const int lab = labels[t_begin + t];
    const float inv_p = 1.f / (float)P;
    for (int r = 0; r < 4; ++r) {
        const int i = 4 * kk + r, q = q0 + i;
        if (q >= Q) continue;
        const float* lg = logits + (size_t)q * C1;
        float mx = lg[0];
        for (int c = 1; c < C1; ++c) mx = fmaxf(mx, lg[c]);
        float den = 0.f;
        for (int c = 0; c < C1; ++c) den += __expf(lg[c] - mx);
        const float prob = (lab >= 0 && lab < C1) ? __expf(lg[lab] - mx) / den : __int_as_float(0x7fc00000);
        const float c_mask = (rows[0][i] - v[r]) * inv_p;
        const float c_dice = 1.f - (2.f * v[4 + r] + 1.f) / (rows[1][i] + rows[2][i16] + 1.f);
        cost[((size_t)pred * Q + q) * TT + t_begin + t] = wm * c_mask + wc * (-prob) + wd * c_dice;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// (b) point losses.  pairs [n_pairs][4]: prediction, row n of that prediction's random points, b * Q + q, global target index.
struct PairView {
    int pred, n, bq, t;
    bool ok;
};

__device__ __forceinline__ PairView cr_pair(const int32_t* __restrict__ pairs, int pair, int n_pred, int N, int BQ, int TT) {
    PairView v;
    v.pred = pairs[4 * pair], v.n = pairs[4 * pair + 1], v.bq = pairs[4 * pair + 2], v.t = pairs[4 * pair + 3];
    v.ok = v.pred >= 0 && v.pred < n_pred && v.n >= 0 && v.n < N && v.bq >= 0 && v.bq < BQ && v.t >= 0 && v.t < TT;
    return v;
}

__device__ __forceinline__ unsigned cr_key(float x) { return __float_as_uint(fabsf(x)); }   // larger -|x| <=> smaller key

__device__ __forceinline__ unsigned long long cr_lanemask_lt(int lane) { return lane == 0 ? 0ull : (~0ull >> (64 - lane)); }

__global__ __launch_bounds__(CR_THREADS) void point_loss_fwd_kernel(const int64_t* __restrict__ table, const uint8_t* __restrict__ tgt,
                                                                    const int32_t* __restrict__ pairs, const float* __restrict__ os_pts,
                                                                    const float* __restrict__ rnd_pts, float4* __restrict__ terms,
                                                                    int32_t* __restrict__ sel_idx, uint32_t* __restrict__ sel_bits,
                                                                    int n_pred, int N, int BQ, int TT, int Hm, int Wm, int Hg, int Wg,
                                                                    int Pos, int k, int P, int words) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sh[2];
    __shared__ int wtot[CR_WAVES];
    __shared__ float red[CR_WAVES][4];
    const int pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PairView pv = cr_pair(pairs, pair, n_pred, N, BQ, TT);
    if (!pv.ok) {                                                                          // uniform over the workgroup
        if (tid == 0) terms[pair] = make_float4(__int_as_float(0x7fc00000), __int_as_float(0x7fc00000), 0.f, 0.f);
        return;
    }
    const float* m = reinterpret_cast<const float*>(table[pv.pred]) + (size_t)pv.bq * Hm * Wm;
    const uint8_t* y = tgt + (size_t)pv.t * Hg * Wg;
    const float* op = os_pts + ((size_t)pv.pred * N + pv.n) * Pos * 2;
    const float* rp = rnd_pts + ((size_t)pv.pred * N + pv.n) * (P - k) * 2;
    int32_t* idx = sel_idx + (size_t)pair * k;

    // radix select of the k smallest keys, 8 bits per pass from the top: prefix = the k-th smallest key, kr = how many keys
    // equal to it belong to the set (the lowest indices among them)
    unsigned prefix = 0, kmask = 0, kr = (unsigned)k;
    if (k > 0) {
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < Pos; i += CR_THREADS) {
                const unsigned key = cr_key(cr_sample(m, Hm, Wm, op[2 * i], op[2 * i + 1]));
                if ((key & kmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned cum = 0;
                int d = 0;
                for (; d < 255; ++d) {
                    if (cum + hist[d] >= kr) break;
                    cum += hist[d];
                }
                sh[0] = prefix | ((unsigned)d << shift);
                sh[1] = kr - cum;
            }
            __syncthreads();
            prefix = sh[0];
            kr = sh[1];
            kmask |= 255u << shift;
        }
    }
    // the set in index order: bitmap words and the compacted index list
    int eq_seen = 0, sel_seen = 0;
    const unsigned long long lt_mask = cr_lanemask_lt(lane);
    for (int base = 0; base < Pos; base += CR_THREADS) {                                   // uniform trip count
        const int i = base + tid;
        bool lt = false, eq = false;
        if (k > 0 && i < Pos) {
            const unsigned key = cr_key(cr_sample(m, Hm, Wm, op[2 * i], op[2 * i + 1]));
            lt = key < prefix;
            eq = key == prefix;
        }
        const unsigned long long be = __ballot(eq);
        if (lane == 0) wtot[wave] = __popcll(be);
        __syncthreads();
        int eq_before = eq_seen, eq_all = 0;
        for (int w = 0; w < CR_WAVES; ++w) {
            if (w < wave) eq_before += wtot[w];
            eq_all += wtot[w];
        }
        const bool sel = lt || (eq && eq_before + __popcll(be & lt_mask) < (int)kr);
        __syncthreads();
        const unsigned long long bs = __ballot(sel);
        if (lane == 0) wtot[wave] = __popcll(bs);
        __syncthreads();
        int sel_before = sel_seen, sel_all = 0;
        for (int w = 0; w < CR_WAVES; ++w) {
            if (w < wave) sel_before += wtot[w];
            sel_all += wtot[w];
        }
        const int pos = sel_before + __popcll(bs & lt_mask);
        if (sel && pos < k) idx[pos] = i;
        const int word = (base + wave * 64) / 32 + (lane >> 5);
        if ((lane & 31) == 0 && word < words) sel_bits[(size_t)pair * words + word] = (uint32_t)(lane ? (bs >> 32) : bs);
        eq_seen += eq_all;
        sel_seen += sel_all;
        __syncthreads();
    }
    __threadfence();                                   // the index list is read back by other waves of this workgroup
    __syncthreads();
    __threadfence();

    float a_ce = 0.f, a_sy = 0.f, a_s = 0.f, a_y = 0.f;
    for (int j = tid; j < P; j += CR_THREADS) {
        float cx, cy;
        if (j < k) {
            const int i = min(max(idx[j], 0), Pos - 1);
            cx = op[2 * i], cy = op[2 * i + 1];
        } else {
            cx = rp[2 * (j - k)], cy = rp[2 * (j - k) + 1];
        }
        const float x = cr_sample(m, Hm, Wm, cx, cy), yy = cr_sample(y, Hg, Wg, cx, cy);
        const float s = cr_sigmoid(x);
        a_ce += cr_softplus(x) - x * yy;               // binary_cross_entropy_with_logits(x, yy)
        a_sy += s * yy;
        a_s += s;
        a_y += yy;
    }
    a_ce = wave_sum(a_ce), a_sy = wave_sum(a_sy), a_s = wave_sum(a_s), a_y = wave_sum(a_y);
    if (lane == 0) {
        red[wave][0] = a_ce, red[wave][1] = a_sy, red[wave][2] = a_s, red[wave][3] = a_y;
    }
    __syncthreads();
    if (tid == 0) {
        float s[4];
        for (int c = 0; c < 4; ++c) {
            s[c] = red[0][c];
            for (int w = 1; w < CR_WAVES; ++w) s[c] += red[w][c];
        }
        const float a = s[1], bb = s[2] + s[3];
        terms[pair] = make_float4(s[0] / (float)P, 1.f - (2.f * a + 1.f) / (bb + 1.f), a, bb);
    }
}

// losses [2][n_pred]: sum over the N masks of each prediction (fixed order) / num_masks
__global__ __launch_bounds__(64) void point_loss_sum_kernel(const float4* __restrict__ terms, float* __restrict__ losses, int n_pred,
                                                            int N, float num_masks) {
    const int pred = blockIdx.x, lane = threadIdx.x;
    float sm = 0.f, sd = 0.f;
    for (int n = lane; n < N; n += 64) {
        const float4 t = terms[(size_t)pred * N + n];
        sm += t.x;
        sd += t.y;
    }
    sm = wave_sum(sm), sd = wave_sum(sd);
    if (lane == 0) {
        losses[pred] = sm / num_masks;
        losses[n_pred + pred] = sd / num_masks;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// (c) backward.  table: [n_pred] mask pointers, [n_pred] gradient pointers (zero-initialised by the caller).
// MODE selects the scatter target at compile time (a pointer that may be either LDS or global memory would be a flat pointer, and
// flat float atomics do not reach LDS):
//   CR_BWD_GLOBAL   float atomics on the gradient in global memory
//   CR_BWD_LDS_F32  the mask's gradient as floats in LDS (float atomics), written out whole
//   CR_BWD_LDS_FIX  the same as 64-bit fixed point: every contribution is scaled by a power of two S chosen per pair from a bound
//                   of the sum (|contribution| <= dmax, at most one per point and pixel, so |sum| <= P dmax < 2^61 / S), rounded
//                   once to an integer and added with INTEGER atomics, so the sum does not depend on arrival order and the
//                   gradient repeats bit for bit; the quantum is 2^-61 of the bound, far below an fp32 ulp of any term that
//                   matters.  A non-finite contribution (nan logits or gradients) makes the whole mask's gradient nan.
enum { CR_BWD_GLOBAL = 0, CR_BWD_LDS_F32 = 1, CR_BWD_LDS_FIX = 2 };

template <int MODE>
__global__ __launch_bounds__(CR_THREADS) void point_loss_bwd_kernel(const int64_t* __restrict__ table, const uint8_t* __restrict__ tgt,
                                                                    const int32_t* __restrict__ pairs, const float* __restrict__ os_pts,
                                                                    const float* __restrict__ rnd_pts, const float4* __restrict__ terms,
                                                                    const int32_t* __restrict__ sel_idx, const float* __restrict__ gl,
                                                                    int n_pred, int N, int BQ, int TT, int Hm, int Wm, int Hg, int Wg,
                                                                    int Pos, int k, int P, float num_masks) {
    extern __shared__ __attribute__((aligned(16))) float acc[];       // LDS_F32: [Hm * Wm] floats; LDS_FIX: [Hm * Wm + 1] 64-bit words
    unsigned long long* acc64 = reinterpret_cast<unsigned long long*>(acc);
    const int pair = blockIdx.x, tid = threadIdx.x;
    const PairView pv = cr_pair(pairs, pair, n_pred, N, BQ, TT);
    if (!pv.ok) return;
    const int HW = Hm * Wm;
    const float* m = reinterpret_cast<const float*>(table[pv.pred]) + (size_t)pv.bq * HW;
    float* g = reinterpret_cast<float*>(table[n_pred + pv.pred]) + (size_t)pv.bq * HW;
    const uint8_t* y = tgt + (size_t)pv.t * Hg * Wg;
    const float* op = os_pts + ((size_t)pv.pred * N + pv.n) * Pos * 2;
    const float* rp = rnd_pts + ((size_t)pv.pred * N + pv.n) * (P - k) * 2;
    const int32_t* idx = sel_idx + (size_t)pair * k;
    const float4 tm = terms[pair];
    const float a = tm.z, bp1 = tm.w + 1.f;
    const float g_ce = gl[pv.pred] / ((float)P * num_masks);
    const float g_d = gl[n_pred + pv.pred] / num_masks;
    const float dnum = 2.f * a + 1.f, dden = bp1 * bp1;
    double scale = 0.0;                                   // LDS_FIX: the power of two S (0: the bound itself is not finite)
    if (MODE == CR_BWD_LDS_FIX) {
        // |d| <= |g_ce| |s - y| + |g_d| |2 y bp1 - dnum| / dden s (1 - s) with |s - y| <= 1, y in [0, 1], s (1 - s) <= 1 / 4
        const double dmax = fabs((double)g_ce) + fabs((double)g_d) * (2.0 * fabs((double)bp1) + fabs((double)dnum)) / (double)dden * 0.25;
        const double bound = (double)P * dmax;
        if (bound > 0.0 && bound < 1.0e300) {
            int e;
            frexp(bound, &e);                             // bound < 2^e
            scale = ldexp(1.0, 61 - e);
        }
        for (int i = tid; i <= HW; i += CR_THREADS) acc64[i] = 0ull;          // [HW]: the non-finite flag
        __syncthreads();
    }
    if (MODE == CR_BWD_LDS_F32) {
        for (int i = tid; i < HW; i += CR_THREADS) acc[i] = 0.f;
        __syncthreads();
    }
    auto add = [&](int i, float v) {
        if (MODE == CR_BWD_LDS_FIX) {
            const double q = (double)v * scale;
            if (fabs(q) < 4.0e18) atomicAdd(acc64 + i, (unsigned long long)__double2ll_rn(q));
            else atomicOr(acc64 + HW, 1ull);              // nan, inf or beyond the bound (a non-finite bound: scale = 0 and q = nan or 0)
        } else if (MODE == CR_BWD_LDS_F32) {
            atomicAdd(acc + i, v);
        } else {
            __hip_atomic_fetch_add(((__attribute__((address_space(1))) float*)g) + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    for (int j = tid; j < P; j += CR_THREADS) {
        float cx, cy;
        if (j < k) {
            const int i = min(max(idx[j], 0), Pos - 1);
            cx = op[2 * i], cy = op[2 * i + 1];
        } else {
            cx = rp[2 * (j - k)], cy = rp[2 * (j - k) + 1];
        }
        const float x = cr_sample(m, Hm, Wm, cx, cy), yy = cr_sample(y, Hg, Wg, cx, cy);
        const float s = cr_sigmoid(x);
        const float d = g_ce * (s - yy) - g_d * (2.f * yy * bp1 - dnum) / dden * s * (1.f - s);
        const float ix = cr_src(cx, Wm), iy = cr_src(cy, Hm);
        const float fx = floorf(ix), fy = floorf(iy);
        const int x0 = (int)fx, y0 = (int)fy;
        const float e = ix - fx, w = (fx + 1.f) - ix, so = iy - fy, n = (fy + 1.f) - iy;
        const bool xa = x0 >= 0 && x0 < Wm, xb = x0 + 1 >= 0 && x0 + 1 < Wm;
        if (y0 >= 0 && y0 < Hm) {
            if (xa) add(y0 * Wm + x0, w * n * d);
            if (xb) add(y0 * Wm + x0 + 1, e * n * d);
        }
        if (y0 + 1 >= 0 && y0 + 1 < Hm) {
            if (xa) add((y0 + 1) * Wm + x0, w * so * d);
            if (xb) add((y0 + 1) * Wm + x0 + 1, e * so * d);
        }
    }
    if (MODE == CR_BWD_LDS_FIX) {
        __syncthreads();
        const bool poisoned = acc64[HW] != 0ull || scale == 0.0 && (g_ce != 0.f || g_d != 0.f);
        const double inv = scale > 0.0 ? 1.0 / scale : 0.0;                   // a power of two: exact
        for (int i = tid; i < HW; i += CR_THREADS)
            g[i] = poisoned ? __int_as_float(0x7fc00000) : (float)((double)(long long)acc64[i] * inv);
    }
    if (MODE == CR_BWD_LDS_F32) {
        __syncthreads();
        for (int i = tid; i < HW; i += CR_THREADS) g[i] = acc[i];
    }
}

bool cr_shape_ok(int Hm, int Wm, int Hg, int Wg) {
    return Hm > 0 && Wm > 0 && Hg > 0 && Wg > 0 && (int64_t)Hm * Wm < (1 << 30) && (int64_t)Hg * Wg < (1 << 30);
}

}  // namespace

extern "C" int msm_match_cost(const int64_t* table, const uint8_t* tgt, const int32_t* labels, const float* points, float* cost,
                              int n_pred, int B, int Q, int C1, int Hm, int Wm, int Hg, int Wg, int P, int TT, int max_T,
                              float w_class, float w_mask, float w_dice, void* stream) {
    MSM_REQUIRE(table && points, "msm_match_cost: null pointer");
    MSM_REQUIRE(n_pred >= 1 && B >= 0 && Q >= 1 && C1 >= 1 && P >= 1 && TT >= 0 && max_T >= 0 && max_T <= TT,
                "msm_match_cost: bad sizes n_pred=%d B=%d Q=%d C1=%d P=%d TT=%d max_T=%d", n_pred, B, Q, C1, P, TT, max_T);
    MSM_REQUIRE(cr_shape_ok(Hm, Wm, Hg, Wg), "msm_match_cost: bad mask sizes %dx%d / %dx%d", Hm, Wm, Hg, Wg);
    MSM_REQUIRE((int64_t)n_pred * B <= 65535, "msm_match_cost: n_pred * B = %lld exceeds the grid", (long long)n_pred * B);
    if (B == 0 || max_T == 0) return MSM_OK;
    MSM_REQUIRE(tgt && labels && cost, "msm_match_cost: null target or cost pointer");
    hipLaunchKernelGGL(match_cost_kernel, dim3(msm::cdiv(Q, 16), msm::cdiv(max_T, 16), n_pred * B), dim3(CR_THREADS), 0,
                       (hipStream_t)stream, table, tgt, labels, points, cost, n_pred, B, Q, C1, Hm, Wm, Hg, Wg, P, TT, w_class,
                       w_mask, w_dice);
    MSM_CHECK_LAUNCH("msm_match_cost");
    return MSM_OK;
}

extern "C" int64_t msm_point_loss_workspace(int n_pairs, int k) {
    if (n_pairs < 0 || k < 0) return -1;
    return (int64_t)n_pairs * 16 + (int64_t)n_pairs * k * 4;
}

extern "C" int msm_point_loss_fwd(const int64_t* table, const uint8_t* tgt, const int32_t* pairs, const float* os_points,
                                  const float* rnd_points, float* losses, uint32_t* sel_bits, void* workspace, int64_t workspace_bytes,
                                  int n_pred, int N, int BQ, int TT, int Hm, int Wm, int Hg, int Wg, int Pos, int k, int P,
                                  float num_masks, void* stream) {
    MSM_REQUIRE(table && losses, "msm_point_loss_fwd: null pointer");
    MSM_REQUIRE(n_pred >= 1 && N >= 0 && BQ >= 1 && TT >= 0 && P >= 1 && k >= 0 && k <= P && k <= Pos && Pos >= 1,
                "msm_point_loss_fwd: bad sizes n_pred=%d N=%d BQ=%d TT=%d Pos=%d k=%d P=%d", n_pred, N, BQ, TT, Pos, k, P);
    MSM_REQUIRE(cr_shape_ok(Hm, Wm, Hg, Wg), "msm_point_loss_fwd: bad mask sizes %dx%d / %dx%d", Hm, Wm, Hg, Wg);
    MSM_REQUIRE(num_masks > 0.f, "msm_point_loss_fwd: num_masks must be positive");
    const int64_t n_pairs = (int64_t)n_pred * N;
    MSM_REQUIRE(n_pairs < (1ll << 31), "msm_point_loss_fwd: too many pairs");
    MSM_REQUIRE(workspace_bytes >= msm_point_loss_workspace((int)n_pairs, k), "msm_point_loss_fwd: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)msm_point_loss_workspace((int)n_pairs, k));
    hipStream_t s = (hipStream_t)stream;
    if (n_pairs > 0) {
        MSM_REQUIRE(tgt && pairs && os_points && rnd_points && sel_bits && workspace, "msm_point_loss_fwd: null pointer");
        float4* terms = static_cast<float4*>(workspace);
        int32_t* idx = reinterpret_cast<int32_t*>(terms + n_pairs);
        hipLaunchKernelGGL(point_loss_fwd_kernel, dim3((unsigned)n_pairs), dim3(CR_THREADS), 0, s, table, tgt, pairs, os_points, rnd_points,
                           terms, idx, sel_bits, n_pred, N, BQ, TT, Hm, Wm, Hg, Wg, Pos, k, P, msm::cdiv(Pos, 32));
        hipLaunchKernelGGL(point_loss_sum_kernel, dim3(n_pred), dim3(64), 0, s, terms, losses, n_pred, N, num_masks);
    } else {
        MSM_CHECK_HIP(hipMemsetAsync(losses, 0, sizeof(float) * 2 * n_pred, s));
    }
    MSM_CHECK_LAUNCH("msm_point_loss_fwd");
    return MSM_OK;
}

extern "C" int msm_point_loss_bwd(const int64_t* table, const uint8_t* tgt, const int32_t* pairs, const float* os_points,
                                  const float* rnd_points, const void* workspace, int64_t workspace_bytes, const float* grad_losses,
                                  int n_pred, int N, int BQ, int TT, int Hm, int Wm, int Hg, int Wg, int Pos, int k, int P,
                                  float num_masks, int flags, void* stream) {
    MSM_REQUIRE(table && grad_losses, "msm_point_loss_bwd: null pointer");
    MSM_REQUIRE(n_pred >= 1 && N >= 0 && BQ >= 1 && TT >= 0 && P >= 1 && k >= 0 && k <= P && k <= Pos && Pos >= 1,
                "msm_point_loss_bwd: bad sizes n_pred=%d N=%d BQ=%d TT=%d Pos=%d k=%d P=%d", n_pred, N, BQ, TT, Pos, k, P);
    MSM_REQUIRE(cr_shape_ok(Hm, Wm, Hg, Wg), "msm_point_loss_bwd: bad mask sizes %dx%d / %dx%d", Hm, Wm, Hg, Wg);
    MSM_REQUIRE(num_masks > 0.f, "msm_point_loss_bwd: num_masks must be positive");
    const int64_t n_pairs = (int64_t)n_pred * N;
    MSM_REQUIRE(n_pairs < (1ll << 31), "msm_point_loss_bwd: too many pairs");
    MSM_REQUIRE(workspace_bytes >= msm_point_loss_workspace((int)n_pairs, k), "msm_point_loss_bwd: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)msm_point_loss_workspace((int)n_pairs, k));
    if (n_pairs == 0) return MSM_OK;
    MSM_REQUIRE(tgt && pairs && os_points && rnd_points && workspace, "msm_point_loss_bwd: null pointer");
    const float4* terms = static_cast<const float4*>(workspace);
    const int32_t* idx = reinterpret_cast<const int32_t*>(terms + n_pairs);
    const int64_t fix_bytes = ((int64_t)Hm * Wm + 1) * 8, f32_bytes = (int64_t)Hm * Wm * 4;
    const bool lds = (flags & MSM_POINT_LOSS_GLOBAL_ATOMICS) == 0;
    hipStream_t s = (hipStream_t)stream;
#define MSM_PL_BWD(MODE, BYTES)                                                                                                     \
    hipLaunchKernelGGL(point_loss_bwd_kernel<MODE>, dim3((unsigned)n_pairs), dim3(CR_THREADS), (size_t)(BYTES), s, table, tgt, pairs, \
                       os_points, rnd_points, terms, idx, grad_losses, n_pred, N, BQ, TT, Hm, Wm, Hg, Wg, Pos, k, P, num_masks)
    if (lds && fix_bytes <= CR_LDS_FIX_MAX) {              // reproducible: masks up to 20 479 pixels (120 x 160 among them)
        MSM_CHECK_HIP((hipError_t)msm::ensure_dynamic_lds((const void*)point_loss_bwd_kernel<CR_BWD_LDS_FIX>, (size_t)fix_bytes));
        MSM_PL_BWD(CR_BWD_LDS_FIX, fix_bytes);
    } else if (lds && f32_bytes <= CR_LDS_MAX) {
        MSM_CHECK_HIP((hipError_t)msm::ensure_dynamic_lds((const void*)point_loss_bwd_kernel<CR_BWD_LDS_F32>, (size_t)f32_bytes));
        MSM_PL_BWD(CR_BWD_LDS_F32, f32_bytes);
    } else {
        MSM_PL_BWD(CR_BWD_GLOBAL, 0);
    }
#undef MSM_PL_BWD
    MSM_CHECK_LAUNCH("msm_point_loss_bwd");
    return MSM_OK;
}
