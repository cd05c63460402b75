// Backward of the two operators of the pixel decoder that are not row-local (see include/msm_hip.h: msm_groupnorm_bwd_f32,
// msm_upsample_bilinear_bwd_tokens_f32): GroupNorm over a token map and the bilinear FPN upsampling.
//
// GroupNorm (reference: torch autograd through nn.GroupNorm(32, 64) of input_proj / adapter_1 / layer_1, msdeformattn.py:216-219,
// 266-281).  With xh = (x - mean) * rstd, y = gamma * xh + beta, g = gout (times [y > 0] behind a ReLU), n = HW * C / groups:
//     dbeta[c]  = sum_{b,p} g                         dgamma[c] = sum_{b,p} g * xh
//     dx        = rstd * (gamma * g - (a + xh * b) / n),   a = sum_{group} gamma * sum_p g,   b = sum_{group} gamma * sum_p g * xh
// Pixels of an image are cut into S ranges (the `splits`).  Three launches on one stream:
//   pass 1   workgroup (range, image): sum_p g and sum_p g * xh per channel -> workspace [B][S][2][C]
//   pass 2   workgroup (range, image): adds the S ranges of its image in index order, forms a and b of every group, writes dx for its
//            range; the workgroup of range 0 also leaves the image's sums in the workspace [B][2][C]
//   params   dgamma / dbeta: the images' sums added in index order
// mean and rstd come from the forward's float64 moments.  Every sum and the dx expression are evaluated in double (inputs and
// outputs are fp32): a + xh * b cancels gamma * g almost completely when a group holds few values (two values: all but eps / var of
// it), and the kernels are bound by their 4 reads + 1 write of the map, not by the ~10 fp64 operations per element.  The ReLU mask
// is the forward's own fp32 expression (gn_apply_kernel, norm.hip), so both passes agree with it on the sign.
// No atomics, no hand-off between workgroups: bit-identical from call to call for a given (shape, splits).
//
// Upsampling: gather form of the adjoint of gn_apply_kernel's `up` term (F.interpolate(mode="bilinear", align_corners=False),
// msdeformattn.py:349).  A thread owns four channels of one low-resolution pixel and walks the high-resolution rows and columns whose
// taps can touch it (a conservative index range; each candidate is then decided by the forward's bilin_src arithmetic itself).
#include "common.h"

namespace msm {

constexpr int GB_T = 256;                // threads per workgroup
constexpr int GB_MAX_SPLITS = 4096;
constexpr int GB_PER = 256;              // pixels per range when the caller leaves the choice to the library

struct GnChan {                          // one channel's constants
    double mean, rstd;
    float mn, sc, sh;                    // the forward's fp32 form: y = (x - mn) * sc + sh
};

// mean / rstd of channel c's group of image b from the float64 moments, as gn_apply_kernel derives them
__device__ __forceinline__ GnChan gn_channel(const double* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ beta,
                                             int b, int c, int C, int cpg, int HW, float eps) {
    const int g0 = (c / cpg) * cpg;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < cpg; ++k) {
        s += stats[((int64_t)b * C + g0 + k) * 2];
        q += stats[((int64_t)b * C + g0 + k) * 2 + 1];
    }
    const double cnt = (double)cpg * (double)HW;
    const double mean = s / cnt;
    double var = q / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    GnChan r;
    r.mean = mean;
    r.rstd = 1.0 / sqrt(var + (double)eps);
    r.mn = (float)mean;
    r.sc = (float)r.rstd * gamma[c];
    r.sh = beta[c];
    return r;
}

// pass 1.  Thread = four channels (c4) of the pixels p0 + st, p0 + st + streams, ...: a workgroup reads whole 16-byte-aligned rows.
__global__ __launch_bounds__(GB_T) void gn_bwd_partial_kernel(const float* __restrict__ x, const float* __restrict__ gout,
                                                              const double* __restrict__ stats, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, double* __restrict__ part, int HW, int C,
                                                              int groups, float eps, int relu, int S, int per) {
    __shared__ GnChan ch[256];
    __shared__ double red[2][4][GB_T];
    const int tid = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
    const int cpg = C / groups;
    if (tid < C) ch[tid] = gn_channel(stats, gamma, beta, b, tid, C, cpg, HW, eps);
    __syncthreads();
    const int c4n = C >> 2, streams = GB_T / c4n;
    const int c4 = tid % c4n, st = tid / c4n;
    const int p0 = min(HW, s * per), p1 = min(HW, p0 + per);
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    if (st < streams) {
        GnChan k[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) k[e] = ch[c4 * 4 + e];
        const int64_t base = (int64_t)b * HW * C + c4 * 4;
        for (int p = p0 + st; p < p1; p += streams) {
            const float4 xv = *reinterpret_cast<const float4*>(x + base + (int64_t)p * C);
            const float4 gv = *reinterpret_cast<const float4*>(gout + base + (int64_t)p * C);
            const float xe[4] = {xv.x, xv.y, xv.z, xv.w}, ge[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool on = !relu || (xe[e] - k[e].mn) * k[e].sc + k[e].sh > 0.f;
                const double g = on ? (double)ge[e] : 0.0;
                s1[e] += g;
                s2[e] = fma(g, ((double)xe[e] - k[e].mean) * k[e].rstd, s2[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        red[0][e][tid] = s1[e];
        red[1][e][tid] = s2[e];
    }
    __syncthreads();
    if (tid < C) {
        const int cc = tid >> 2, e = tid & 3;
        double a = 0.0, q = 0.0;
        for (int j = 0; j < streams; ++j) {
            a += red[0][e][j * c4n + cc];
            q += red[1][e][j * c4n + cc];
        }
        double* o = part + ((int64_t)b * S + s) * 2 * C;
        o[tid] = a;
        o[C + tid] = q;
    }
}

// pass 2.  dx == nullptr: only the image sums (grid.x == 1).
__global__ __launch_bounds__(GB_T) void gn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ gout,
                                                            const double* __restrict__ stats, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const double* __restrict__ part,
                                                            double* __restrict__ img, float* __restrict__ dx, int HW, int C, int groups,
                                                            float eps, int relu, int S, int per) {
    __shared__ GnChan ch[256];
    __shared__ double sums[2][256];          // the image's sum_p g, sum_p g * xh per channel
    __shared__ double ga[256], gb[256];      // a / n and b / n of the channel's group
    const int tid = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
    const int cpg = C / groups;
    if (tid < C) ch[tid] = gn_channel(stats, gamma, beta, b, tid, C, cpg, HW, eps);
    for (int t = tid; t < 2 * C; t += GB_T) {
        const double* pp = part + (int64_t)b * S * 2 * C + t;
        double a = 0.0;
        for (int j = 0; j < S; ++j) a += pp[(int64_t)j * 2 * C];
        sums[t / C][t % C] = a;
        if (s == 0) img[(int64_t)b * 2 * C + t] = a;
    }
    __syncthreads();
    if (!dx) return;
    if (tid < C) {
        const int g0 = (tid / cpg) * cpg;
        double a = 0.0, q = 0.0;
        for (int k = 0; k < cpg; ++k) {
            a = fma((double)gamma[g0 + k], sums[0][g0 + k], a);
            q = fma((double)gamma[g0 + k], sums[1][g0 + k], q);
        }
        const double n = (double)cpg * (double)HW;
        ga[tid] = a / n;
        gb[tid] = q / n;
    }
    __syncthreads();
    const int c4n = C >> 2, streams = GB_T / c4n;
    const int c4 = tid % c4n, st = tid / c4n;
    if (st >= streams) return;
    const int p0 = min(HW, s * per), p1 = min(HW, p0 + per);
    GnChan k[4];
    double gm[4], ka[4], kb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        k[e] = ch[c4 * 4 + e];
        gm[e] = (double)gamma[c4 * 4 + e];
        ka[e] = ga[c4 * 4 + e];
        kb[e] = gb[c4 * 4 + e];
    }
    const int64_t base = (int64_t)b * HW * C + c4 * 4;
    for (int p = p0 + st; p < p1; p += streams) {
        const float4 xv = *reinterpret_cast<const float4*>(x + base + (int64_t)p * C);
        const float4 gv = *reinterpret_cast<const float4*>(gout + base + (int64_t)p * C);
        const float xe[4] = {xv.x, xv.y, xv.z, xv.w}, ge[4] = {gv.x, gv.y, gv.z, gv.w};
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool on = !relu || (xe[e] - k[e].mn) * k[e].sc + k[e].sh > 0.f;
            const double g = on ? (double)ge[e] : 0.0;
            const double xh = ((double)xe[e] - k[e].mean) * k[e].rstd;
            o[e] = (float)(k[e].rstd * (gm[e] * g - (ka[e] + xh * kb[e])));
        }
        *reinterpret_cast<float4*>(dx + base + (int64_t)p * C) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// dbeta[c] / dgamma[c]: the images' sums in index order
__global__ __launch_bounds__(GB_T) void gn_bwd_params_kernel(const double* __restrict__ img, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta, int B, int C) {
    const int t = blockIdx.x * GB_T + threadIdx.x;
    if (t >= 2 * C) return;
    float* out = t < C ? dbeta : dgamma;
    if (!out) return;
    double a = 0.0;
    for (int b = 0; b < B; ++b) a += img[(int64_t)b * 2 * C + t];
    out[t % C] = (float)a;
}

static int gn_bwd_splits(int HW, int splits) { return splits > 0 ? splits : min(GB_MAX_SPLITS, cdiv(HW, GB_PER)); }

static bool gn_bwd_shape_ok(int B, int HW, int C, int groups, int splits) {
    return B > 0 && B <= 65535 && HW > 0 && groups > 0 && C > 0 && C <= 256 && C % 4 == 0 && C % groups == 0 && splits >= 0 &&
           splits <= GB_MAX_SPLITS && (int64_t)HW + GB_MAX_SPLITS < ((int64_t)1 << 31);
}

#define GB_SHAPE_MSG "need 1 <= B <= 65535, HW >= 1, C a multiple of 4 and of groups up to 256 and 0 <= splits <= %d (B=%d HW=%d C=%d groups=%d splits=%d)"

// PyTorch area_pixel_compute_source_index, align_corners=False: the forward's arithmetic (bilin_src in norm.hip)
__device__ __forceinline__ void up_src(int dst, float scale, int in, int& i0, int& i1, float& l1) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = (int)src;
    i1 = i0 + ((i0 < in - 1) ? 1 : 0);
    l1 = src - (float)i0;
}

// the weight of low-resolution index `i` in the forward's taps of high-resolution index `dst`
__device__ __forceinline__ float up_weight(int dst, float scale, int in, int i) {
    int i0, i1;
    float l1;
    up_src(dst, scale, in, i0, i1, l1);
    return (i0 == i ? 1.f - l1 : 0.f) + (i1 == i ? l1 : 0.f);
}

// high-resolution indices whose source coordinate can lie in [i - 1, i + 1): the exact bounds widened by two on each side
__device__ __forceinline__ void up_range(int i, int in, int out, int& lo, int& hi) {
    const double r = (double)out / (double)in;
    lo = max(0, (int)floor(((double)i - 0.5) * r - 0.5) - 2);
    hi = min(out - 1, (int)ceil(((double)i + 1.5) * r - 0.5) + 2);
}

// the forward as an operator of its own (the training graph adds it to the lateral map): thread = four channels of one output pixel,
// the four taps and the expression of gn_apply_kernel's `up` term
__global__ __launch_bounds__(256) void upsample_bilinear_fwd_kernel(const float* __restrict__ in, int64_t in_sb, float* __restrict__ out,
                                                                    int B, int h, int w, int H, int W, int C) {
    const int c4n = C >> 2;
    const int64_t total = (int64_t)B * H * W * c4n;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % c4n) * 4;
        const int64_t q = idx / c4n;
        const int b = (int)(q / ((int64_t)H * W)), p = (int)(q - (int64_t)b * H * W);
        const int yy = p / W, xx = p - yy * W;
        int y0, y1, x0, x1;
        float ly, lx;
        up_src(yy, sy, h, y0, y1, ly);
        up_src(xx, sx, w, x0, x1, lx);
        const float* ub = in + (int64_t)b * in_sb + c;
        const float4 v00 = *reinterpret_cast<const float4*>(ub + ((int64_t)y0 * w + x0) * C);
        const float4 v01 = *reinterpret_cast<const float4*>(ub + ((int64_t)y0 * w + x1) * C);
        const float4 v10 = *reinterpret_cast<const float4*>(ub + ((int64_t)y1 * w + x0) * C);
        const float4 v11 = *reinterpret_cast<const float4*>(ub + ((int64_t)y1 * w + x1) * C);
        const float hy = 1.f - ly, hx = 1.f - lx;
        float4 v;
        v.x = hy * (hx * v00.x + lx * v01.x) + ly * (hx * v10.x + lx * v11.x);
        v.y = hy * (hx * v00.y + lx * v01.y) + ly * (hx * v10.y + lx * v11.y);
        v.z = hy * (hx * v00.z + lx * v01.z) + ly * (hx * v10.z + lx * v11.z);
        v.w = hy * (hx * v00.w + lx * v01.w) + ly * (hx * v10.w + lx * v11.w);
        *reinterpret_cast<float4*>(out + q * C + c) = v;
    }
}

__global__ __launch_bounds__(256) void upsample_bilinear_bwd_kernel(const float* __restrict__ gout, float* __restrict__ gin, int B, int h,
                                                                    int w, int H, int W, int C) {
    const int c4n = C >> 2;
    const int64_t total = (int64_t)B * h * w * c4n;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % c4n) * 4;
        const int64_t q = idx / c4n;
        const int b = (int)(q / ((int64_t)h * w)), p = (int)(q - (int64_t)b * h * w);
        const int iy = p / w, ix = p - iy * w;
        int Y0, Y1, X0, X1;
        up_range(iy, h, H, Y0, Y1);
        up_range(ix, w, W, X0, X1);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        const float* gb = gout + (int64_t)b * H * W * C + c;
        for (int Y = Y0; Y <= Y1; ++Y) {
            const float wy = up_weight(Y, sy, h, iy);
            if (wy == 0.f) continue;
            for (int X = X0; X <= X1; ++X) {
                const float wx = up_weight(X, sx, w, ix);
                if (wx == 0.f) continue;
                const float4 g = *reinterpret_cast<const float4*>(gb + ((int64_t)Y * W + X) * C);
                const float wt = wy * wx;
                acc.x = fmaf(wt, g.x, acc.x);
                acc.y = fmaf(wt, g.y, acc.y);
                acc.z = fmaf(wt, g.z, acc.z);
                acc.w = fmaf(wt, g.w, acc.w);
            }
        }
        *reinterpret_cast<float4*>(gin + q * C + c) = acc;
    }
}

}  // namespace msm

using namespace msm;

extern "C" int64_t msm_groupnorm_bwd_workspace(int B, int HW, int C, int groups, int splits) {
    if (!gn_bwd_shape_ok(B, HW, C, groups, splits)) {
        set_error("msm_groupnorm_bwd_workspace: " GB_SHAPE_MSG, GB_MAX_SPLITS, B, HW, C, groups, splits);
        return MSM_E_INVALID;
    }
    // doubles: [B][S][2][C] range sums + [B][2][C] image sums, counted in floats
    return 2 * ((int64_t)B * gn_bwd_splits(HW, splits) * 2 * C + (int64_t)B * 2 * C);
}

extern "C" int msm_groupnorm_bwd_f32(const float* x, const float* gout, const double* stats, const float* gamma, const float* beta,
                                     float* dx, float* dgamma, float* dbeta, float* workspace, int B, int HW, int C, int groups,
                                     float eps, int relu, int splits, void* stream) {
    MSM_REQUIRE(x && gout && stats && gamma && beta && workspace, "msm_groupnorm_bwd_f32: null pointer");
    MSM_REQUIRE(gn_bwd_shape_ok(B, HW, C, groups, splits), "msm_groupnorm_bwd_f32: " GB_SHAPE_MSG, GB_MAX_SPLITS, B, HW, C, groups, splits);
    MSM_REQUIRE(((((uintptr_t)x) | ((uintptr_t)gout) | ((uintptr_t)dx) | ((uintptr_t)workspace)) & 15) == 0 &&
                    ((((uintptr_t)gamma) | ((uintptr_t)beta) | ((uintptr_t)dgamma) | ((uintptr_t)dbeta)) & 3) == 0 &&
                    (((uintptr_t)stats) & 7) == 0,
                "msm_groupnorm_bwd_f32: misaligned pointer");
    if (!dx && !dgamma && !dbeta) return MSM_OK;
    const int S = gn_bwd_splits(HW, splits);
    const int per = cdiv(HW, S);
    double* part = reinterpret_cast<double*>(workspace);
    double* img = part + (int64_t)B * S * 2 * C;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gn_bwd_partial_kernel, dim3(S, B), dim3(GB_T), 0, st, x, gout, stats, gamma, beta, part, HW, C, groups, eps, relu, S,
                       per);
    MSM_CHECK_LAUNCH("msm_groupnorm_bwd_f32(partial sums)");
    hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3(dx ? S : 1, B), dim3(GB_T), 0, st, x, gout, stats, gamma, beta, part, img, dx, HW, C,
                       groups, eps, relu, S, per);
    MSM_CHECK_LAUNCH("msm_groupnorm_bwd_f32(dx)");
    if (dgamma || dbeta) {
        hipLaunchKernelGGL(gn_bwd_params_kernel, dim3(cdiv(2 * C, GB_T)), dim3(GB_T), 0, st, img, dgamma, dbeta, B, C);
        MSM_CHECK_LAUNCH("msm_groupnorm_bwd_f32(dgamma, dbeta)");
    }
    return MSM_OK;
}

#define UP_SHAPE_OK \
    (B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && (int64_t)h * w < ((int64_t)1 << 31) && (int64_t)H * W < ((int64_t)1 << 31))

extern "C" int msm_upsample_bilinear_tokens_f32(const float* in, int64_t in_batch_stride, float* out, int B, int h, int w, int H, int W,
                                                int C, void* stream) {
    MSM_REQUIRE(in && out, "msm_upsample_bilinear_tokens_f32: null pointer");
    MSM_REQUIRE(UP_SHAPE_OK, "msm_upsample_bilinear_tokens_f32: need B, h, w, H, W >= 1 and C a multiple of 4 (B=%d h=%d w=%d H=%d W=%d C=%d)", B,
                h, w, H, W, C);
    if (in_batch_stride == 0) in_batch_stride = (int64_t)h * w * C;
    MSM_REQUIRE(in_batch_stride >= (int64_t)h * w * C && in_batch_stride % 4 == 0, "msm_upsample_bilinear_tokens_f32: bad batch stride");
    MSM_REQUIRE(((((uintptr_t)in) | ((uintptr_t)out)) & 15) == 0, "msm_upsample_bilinear_tokens_f32: pointers must be 16-byte aligned");
    const int64_t total = (int64_t)B * H * W * (C / 4);
    hipLaunchKernelGGL(upsample_bilinear_fwd_kernel, dim3((unsigned)min((int64_t)4096, (total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, in, in_batch_stride, out, B, h, w, H, W, C);
    MSM_CHECK_LAUNCH("msm_upsample_bilinear_tokens_f32");
    return MSM_OK;
}

extern "C" int msm_upsample_bilinear_bwd_tokens_f32(const float* gout, float* gin, int B, int h, int w, int H, int W, int C,
                                                    void* stream) {
    MSM_REQUIRE(gout && gin, "msm_upsample_bilinear_bwd_tokens_f32: null pointer");
    MSM_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && (int64_t)h * w < ((int64_t)1 << 31) &&
                    (int64_t)H * W < ((int64_t)1 << 31),
                "msm_upsample_bilinear_bwd_tokens_f32: need B, h, w, H, W >= 1 and C a multiple of 4 (B=%d h=%d w=%d H=%d W=%d C=%d)", B, h,
                w, H, W, C);
    MSM_REQUIRE(((((uintptr_t)gout) | ((uintptr_t)gin)) & 15) == 0, "msm_upsample_bilinear_bwd_tokens_f32: pointers must be 16-byte aligned");
    const int64_t total = (int64_t)B * h * w * (C / 4);
    hipLaunchKernelGGL(upsample_bilinear_bwd_kernel, dim3((unsigned)min((int64_t)4096, (total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, gout, gin, B, h, w, H, W, C);
    MSM_CHECK_LAUNCH("msm_upsample_bilinear_bwd_tokens_f32");
    return MSM_OK;
}
