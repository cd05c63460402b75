// Deterministic backward of multi-scale deformable attention (see include/msm_hip.h).
//
// msda_bwd_kernel (msda.hip) scatters grad_value with fp32 atomics: the sum of a destination's contributions is taken in arrival
// order, so its last bits change from run to run.  Here the sum is DEFINED so that it has no order:
//
//   a contribution to destination (image b, pixel s, head m), channel c, is  x = w_k * (go_c * a)  in fp32 (the products and their
//   order are those of msda_bwd_kernel);  the destination has  mx = max over its contributions' (query, point, corner) of
//   w_k * (gmax * |a|), gmax = max_c |go_c| of that (query, head) -- so |x| <= mx for every channel, exactly, because an fp32 product
//   is monotone in each factor -- and cnt = the number of those (query, point, corner);  with
//       k1 = max(exponent field of mx, 1) - 126      (mx < 2^k1),      c = bits(cnt)      (cnt + 1 <= 2^c),      e = 61 - k1 - c
//   grad_value[b][s][m][c] = float( double( sum over the contributions of rne(x * 2^e) ) * 2^-e ).
//
// x * 2^e is exact in double, the integers are summed exactly in int64 (|sum| <= cnt * mx * 2^e < 2^61), and integer addition is
// associative: the result is a pure function of the SET of contributions -- it depends neither on the grid, nor on the order of
// arrival, nor on the order of queries or points, nor on the other images, nor on how the workspace is cut into groups of images.
// (mx, cnt) themselves come from integer atomics (a max on non-negative float bits, a count) and have no order either.
//
// Non-finite: a destination whose mx ranks at or above the bits of +inf (a NaN ranks above every number) received a non-finite
// contribution, or one whose bound overflows; all its D channels are NaN and nothing is accumulated for it.
//
// grad_sampling_loc / grad_attn_weight belong to one (query, head, level, point): the head's D/V lanes are padded with idle lanes
// to the next power of two, so that a head sits inside one wave, and summed by the shuffle butterfly of msda_bwd_kernel -- a fixed
// association, no atomics and no zero-fill; when D/V is a power of two the lane mapping and the arithmetic are msda_bwd_kernel's.
//
// Launches per group of images: a kernel that zeroes the group's workspace, scale pass, accumulate pass, finish pass (kernels only:
// the same four nodes in a captured graph as on a stream).
#include "common.h"

namespace msm {

namespace {

constexpr int DET_MAXL = 8;
constexpr unsigned DET_INF_BITS = 0x7f800000u;

struct DetEntry {            // per destination (image, pixel, head): 8 bytes
    unsigned mx_bits;        // max of the contributions' bound, as the bits of a non-negative float
    unsigned cnt;            // number of (query, point, corner) that hit the destination
};

__device__ __forceinline__ int det_exponent(unsigned mx_bits, unsigned cnt) {   // cnt >= 1, mx finite
    const int E = (int)(mx_bits >> 23);
    const int k1 = (E > 1 ? E : 1) - 126;
    const int c = 32 - __clz((int)cnt);
    return 61 - k1 - c;
}
__device__ __forceinline__ double det_pow2(int e) {                             // 2^e, -1022 <= e <= 1023
    return __longlong_as_double((long long)(e + 1023) << 52);
}

template <int V>
struct DVec {
    float e[V];
};
template <int V>
__device__ __forceinline__ DVec<V> dldv(const float* p) {
    DVec<V> r;
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        r.e[0] = t.x; r.e[1] = t.y; r.e[2] = t.z; r.e[3] = t.w;
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) r.e[i] = p[i];
    }
    return r;
}

// The tap geometry of one sampling point (msda_bwd_kernel's arithmetic): ONE function, inlined into the scale pass and the
// accumulate pass, so that both see the same cell, the same validity and the same four weights for a point.
struct DetTaps {
    bool inside, ok1, ok2, ok3, ok4;
    int h_low, w_low;
    float lh, lw, hh, hw, w1, w2, w3, w4;
};
__device__ __forceinline__ DetTaps det_taps(float loc_x, float loc_y, int H, int W) {
    DetTaps t;
    const float h_im = loc_y * (float)H - 0.5f;
    const float w_im = loc_x * (float)W - 0.5f;
    t.inside = h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W;
    t.h_low = (int)floorf(h_im);
    t.w_low = (int)floorf(w_im);
    t.lh = h_im - (float)t.h_low;
    t.lw = w_im - (float)t.w_low;
    t.hh = 1.f - t.lh;
    t.hw = 1.f - t.lw;
    t.ok1 = t.inside && t.h_low >= 0 && t.w_low >= 0;
    t.ok2 = t.inside && t.h_low >= 0 && t.w_low + 1 <= W - 1;
    t.ok3 = t.inside && t.h_low + 1 <= H - 1 && t.w_low >= 0;
    t.ok4 = t.inside && t.h_low + 1 <= H - 1 && t.w_low + 1 <= W - 1;
    t.w1 = t.hh * t.hw;
    t.w2 = t.hh * t.lw;
    t.w3 = t.lh * t.hw;
    t.w4 = t.lh * t.lw;
    return t;
}

// ---- zero the group's workspace (8-byte words) -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void msda_det_zero_kernel(unsigned long long* __restrict__ ws, int64_t words) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) ws[i] = 0ull;
}

// ---- scale pass: one lane per (image of the group, query, head) ----------------------------------------------------------------
__global__ __launch_bounds__(256) void msda_det_scale_kernel(const int64_t* __restrict__ shapes, const int64_t* __restrict__ lstart,
                                                             const float* __restrict__ loc, const float* __restrict__ wgt,
                                                             const float* __restrict__ gout, DetEntry* __restrict__ table, int b0, int G,
                                                             int S, int M, int D, int L, int Lq, int P) {
    const int64_t per_img = (int64_t)Lq * M;
    const int g = blockIdx.x % G;
    const int64_t idx = (int64_t)(blockIdx.x / G) * 256 + threadIdx.x;
    if (idx >= per_img) return;
    const int m = (int)(idx % M);
    const int qi = (int)(idx / M);
    const int b = b0 + g;
    const float* gp = gout + (((int64_t)b * Lq + qi) * M + m) * D;
    unsigned gbits = 0;                                       // max on the bits of |go_c|: a NaN ranks above every number
    for (int c = 0; c < D; ++c) {
        const unsigned v = __float_as_uint(gp[c]) & 0x7fffffffu;
        gbits = v > gbits ? v : gbits;
    }
    const float gmax = __uint_as_float(gbits);
    const int64_t base = (((int64_t)b * Lq + qi) * M + m) * L * P;
    DetEntry* tb = table + (int64_t)g * S * M + m;
    for (int l = 0; l < L; ++l) {
        const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
        const int64_t s0 = lstart[l];
        for (int p = 0; p < P; ++p) {
            const int i = l * P + p;
            const float loc_x = loc[(base + i) * 2], loc_y = loc[(base + i) * 2 + 1], aw = wgt[base + i];
            const DetTaps t = det_taps(loc_x, loc_y, H, W);
            if (!t.inside) continue;
            const float tb_abs = gmax * fabsf(aw);            // >= |go_c * aw| for every channel c, exactly
            const int64_t s1 = s0 + (int64_t)t.h_low * W + t.w_low;
#define MSDA_DET_MARK(ok, s, w)                                                           \
    if (ok) {                                                                             \
        DetEntry* en = tb + (s) * M;                                                      \
        /* (tried: a plain read first, skipping the max where it cannot change the entry -- slower, 4.77 against 4.38 ms per call at */ \
        /* B = 8: the no-return atomics are fire-and-forget, a read makes the lane wait for memory) */ \
        atomicMax(&en->mx_bits, __float_as_uint((w) * tb_abs) & 0x7fffffffu);            \
        atomicAdd(&en->cnt, 1u);                                                          \
    }
            MSDA_DET_MARK(t.ok1, s1, t.w1)
            MSDA_DET_MARK(t.ok2, s1 + 1, t.w2)
            MSDA_DET_MARK(t.ok3, s1 + W, t.w3)
            MSDA_DET_MARK(t.ok4, s1 + W + 1, t.w4)
#undef MSDA_DET_MARK
        }
    }
}

// ---- accumulate pass: msda_bwd_kernel's arithmetic; a head's D/V lanes padded to PD4 = the next power of two ------------------------
template <int V>
__global__ __launch_bounds__(256) void msda_det_accum_kernel(const float* __restrict__ value, const int64_t* __restrict__ shapes,
                                                             const int64_t* __restrict__ lstart, const float* __restrict__ loc,
                                                             const float* __restrict__ wgt, const float* __restrict__ gout,
                                                             const DetEntry* __restrict__ table, unsigned long long* __restrict__ acc,
                                                             float* __restrict__ gloc, float* __restrict__ gwgt, int b0, int G, int S,
                                                             int M, int D, int L, int Lq, int P, int PD4) {
    const int D4 = D / V;
    const int64_t per_img = (int64_t)Lq * M * PD4;
    const int g = blockIdx.x % G;
    const int64_t idx = (int64_t)(blockIdx.x / G) * 256 + threadIdx.x;
    // PD4 <= 64 divides 256: a head is never split by a wave, a workgroup or the bound below; idle lanes shuffle zeros
    const int64_t cidx = idx < per_img ? idx : 0;
    const int d4 = (int)(cidx % PD4);
    const bool live = idx < per_img && d4 < D4;
    const int dl = live ? d4 : 0;
    const int64_t t = cidx / PD4;
    const int m = (int)(t % M);
    const int qi = (int)(t / M);
    const int b = b0 + g;

    const int64_t pix_stride = (int64_t)M * D;
    const int64_t voff = (int64_t)b * S * pix_stride + m * D + dl * V;
    const DetEntry* tb = table + (int64_t)g * S * M + m;
    unsigned long long* ab = acc + (int64_t)g * S * pix_stride + m * D + dl * V;
    const DVec<V> go = dldv<V>(gout + (((int64_t)b * Lq + qi) * M + m) * D + dl * V);
    const int64_t base = (((int64_t)b * Lq + qi) * M + m) * L * P;
    for (int l = 0; l < L; ++l) {
        const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
        const int64_t s0 = lstart[l];
        const int64_t lvl = voff + s0 * pix_stride;
        for (int p = 0; p < P; ++p) {
            const int i = l * P + p;
            const float loc_x = loc[(base + i) * 2], loc_y = loc[(base + i) * 2 + 1], aw = wgt[base + i];
            const DetTaps t = det_taps(loc_x, loc_y, H, W);
            float g_w = 0.f, g_x = 0.f, g_y = 0.f;
            if (live && t.inside) {
                const int h_low = t.h_low, w_low = t.w_low;
                const float lh = t.lh, lw = t.lw, hh = t.hh, hw = t.hw;
                const bool ok1 = t.ok1, ok2 = t.ok2, ok3 = t.ok3, ok4 = t.ok4;
                const int64_t s1 = s0 + (int64_t)h_low * W + w_low, s2 = s1 + 1, s3 = s1 + W, s4 = s3 + 1;
                const int64_t o1 = lvl + ((int64_t)h_low * W + w_low) * pix_stride, o2 = o1 + pix_stride;
                const int64_t o3 = o1 + (int64_t)W * pix_stride, o4 = o3 + pix_stride;
                DVec<V> v1, v2, v3, v4;
#pragma unroll
                for (int c = 0; c < V; ++c) v1.e[c] = v2.e[c] = v3.e[c] = v4.e[c] = 0.f;
                // the destination's scale: 2^e, or 0 where it is marked non-finite (nothing is accumulated there)
                double sc1 = 0.0, sc2 = 0.0, sc3 = 0.0, sc4 = 0.0;
#define MSDA_DET_TAP(ok, v, o, s, sc)                                                       \
    if (ok) {                                                                               \
        v = dldv<V>(value + (o));                                                           \
        const DetEntry en = tb[(s) * M];                                                    \
        if (en.mx_bits < DET_INF_BITS) sc = det_pow2(det_exponent(en.mx_bits, en.cnt));     \
    }
                MSDA_DET_TAP(ok1, v1, o1, s1, sc1)
                MSDA_DET_TAP(ok2, v2, o2, s2, sc2)
                MSDA_DET_TAP(ok3, v3, o3, s3, sc3)
                MSDA_DET_TAP(ok4, v4, o4, s4, sc4)
#undef MSDA_DET_TAP
                const float w1 = t.w1, w2 = t.w2, w3 = t.w3, w4 = t.w4;
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    const float tg = go.e[c] * aw;
                    if (sc1 != 0.0) atomicAdd(ab + s1 * pix_stride + c, (unsigned long long)__double2ll_rn((double)(w1 * tg) * sc1));
                    if (sc2 != 0.0) atomicAdd(ab + s2 * pix_stride + c, (unsigned long long)__double2ll_rn((double)(w2 * tg) * sc2));
                    if (sc3 != 0.0) atomicAdd(ab + s3 * pix_stride + c, (unsigned long long)__double2ll_rn((double)(w3 * tg) * sc3));
                    if (sc4 != 0.0) atomicAdd(ab + s4 * pix_stride + c, (unsigned long long)__double2ll_rn((double)(w4 * tg) * sc4));
                    g_w += go.e[c] * (w1 * v1.e[c] + w2 * v2.e[c] + w3 * v3.e[c] + w4 * v4.e[c]);
                    g_x += tg * (-hh * v1.e[c] + hh * v2.e[c] - lh * v3.e[c] + lh * v4.e[c]);
                    g_y += tg * (-hw * v1.e[c] - lw * v2.e[c] + hw * v3.e[c] + lw * v4.e[c]);
                }
                g_x *= (float)W;
                g_y *= (float)H;
            }
            for (int o = PD4 >> 1; o > 0; o >>= 1) {
                g_w += __shfl_xor(g_w, o, 64);
                g_x += __shfl_xor(g_x, o, 64);
                g_y += __shfl_xor(g_y, o, 64);
            }
            if (live && d4 == 0) {
                gwgt[base + i] = g_w;
                gloc[(base + i) * 2] = g_x;
                gloc[(base + i) * 2 + 1] = g_y;
            }
        }
    }
}

// ---- finish pass: int64 -> double -> * 2^-e -> float; every element of the group's grad_value is written -----------------------------
__global__ __launch_bounds__(256) void msda_det_finish_kernel(const DetEntry* __restrict__ table, const long long* __restrict__ acc,
                                                              float* __restrict__ gvalue, int64_t total, int D) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const DetEntry en = table[i / D];
        float r = 0.f;
        if (en.mx_bits >= DET_INF_BITS) r = __uint_as_float(0x7fc00000u);
        else if (en.cnt != 0) r = (float)((double)acc[i] * det_pow2(-det_exponent(en.mx_bits, en.cnt)));
        gvalue[i] = r;
    }
}

int64_t det_image_bytes(int64_t S, int64_t M, int64_t D) { return S * M * 8 * (D + 1); }

}  // namespace

}  // namespace msm

using namespace msm;

extern "C" int64_t msm_msdeform_attn_bwd_det_workspace(int B, int S, int M, int D) {
    if (B <= 0 || S <= 0 || M <= 0 || D <= 0) return 0;
    return (int64_t)B * det_image_bytes(S, M, D);
}

extern "C" int msm_msdeform_attn_bwd_det(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                         const float* sampling_loc, const float* attn_weight, const float* grad_output,
                                         float* grad_value, float* grad_sampling_loc, float* grad_attn_weight, int B, int S, int M,
                                         int D, int L, int Lq, int P, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* name = "msm_msdeform_attn_bwd_det";
    MSM_REQUIRE(value && spatial_shapes && level_start_index && sampling_loc && attn_weight && grad_output && grad_value &&
                    grad_sampling_loc && grad_attn_weight && workspace,
                "%s: null pointer", name);
    MSM_REQUIRE(B > 0 && S > 0 && M > 0 && Lq > 0 && P > 0, "%s: bad sizes", name);
    MSM_REQUIRE(D > 0 && D <= 64 && L > 0 && L <= DET_MAXL,
                "%s: D=%d, L=%d: the deterministic backward covers D <= 64 and L <= %d (float32)", name, D, L, DET_MAXL);
    MSM_REQUIRE(((((uintptr_t)value) | ((uintptr_t)grad_output) | ((uintptr_t)grad_value) | ((uintptr_t)workspace)) & 15) == 0,
                "%s: value, grad_output, grad_value and workspace must be 16-byte aligned", name);
    const int64_t img_bytes = det_image_bytes(S, M, D);
    MSM_REQUIRE(workspace_bytes >= img_bytes, "%s: workspace of %lld bytes is smaller than one image's %lld bytes", name,
                (long long)workspace_bytes, (long long)img_bytes);
    const int V = (D % 4 == 0) ? 4 : 1;
    const int D4 = D / V;
    int PD4 = 1;
    while (PD4 < D4) PD4 *= 2;
    const int64_t Gmax = workspace_bytes / img_bytes;
    const int G0 = (int)(Gmax < B ? Gmax : B);
    const int64_t blk_scale = ((int64_t)Lq * M + 255) / 256, blk_acc = ((int64_t)Lq * M * PD4 + 255) / 256;
    MSM_REQUIRE(blk_acc * G0 < ((int64_t)1 << 31) && (int64_t)S * M * D < ((int64_t)1 << 31), "%s: sizes too large", name);
    hipStream_t st = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += G0) {
        const int G = B - b0 < G0 ? B - b0 : G0;
        DetEntry* table = reinterpret_cast<DetEntry*>(workspace);
        unsigned long long* acc = reinterpret_cast<unsigned long long*>(table + (int64_t)G * S * M);
        const int64_t words = G * img_bytes / 8;
        const int64_t zero_blocks = (words + 255) / 256;
        hipLaunchKernelGGL(msda_det_zero_kernel, dim3((unsigned)(zero_blocks < 8192 ? zero_blocks : 8192)), dim3(256), 0, st,
                           reinterpret_cast<unsigned long long*>(workspace), words);
        hipLaunchKernelGGL(msda_det_scale_kernel, dim3((unsigned)(blk_scale * G)), dim3(256), 0, st, spatial_shapes, level_start_index,
                           sampling_loc, attn_weight, grad_output, table, b0, G, S, M, D, L, Lq, P);
        if (V == 4)
            hipLaunchKernelGGL((msda_det_accum_kernel<4>), dim3((unsigned)(blk_acc * G)), dim3(256), 0, st, value, spatial_shapes,
                               level_start_index, sampling_loc, attn_weight, grad_output, table, acc, grad_sampling_loc,
                               grad_attn_weight, b0, G, S, M, D, L, Lq, P, PD4);
        else
            hipLaunchKernelGGL((msda_det_accum_kernel<1>), dim3((unsigned)(blk_acc * G)), dim3(256), 0, st, value, spatial_shapes,
                               level_start_index, sampling_loc, attn_weight, grad_output, table, acc, grad_sampling_loc,
                               grad_attn_weight, b0, G, S, M, D, L, Lq, P, PD4);
        const int64_t total = (int64_t)G * S * M * D;
        const int64_t fin_blocks = (total + 255) / 256;
        hipLaunchKernelGGL(msda_det_finish_kernel, dim3((unsigned)(fin_blocks < 8192 ? fin_blocks : 8192)), dim3(256), 0, st, table,
                           reinterpret_cast<const long long*>(acc), grad_value + (int64_t)b0 * S * M * D, total, D);
        MSM_CHECK_LAUNCH(name);
    }
    return MSM_OK;
}
