// Weight and bias gradient of the 3x3 / pad 1 convolution of a 64-channel token map (see include/msm_hip.h: msm_conv3x3_c64_wgrad):
//     dw[o][tap*64 + c] = sum_{b,p} g[b][o][p] * x[b][p + tap][c]        (taps outside the image contribute nothing)
//     dbias[o]          = sum_{b,p} g[b][o][p]
// x: the NHWC token map [B][H*W][64] the forward read, g: the gradient of the NCHW output [B][Cout][H*W].
//
// Reference: torch autograd through SimpleBasePixelDecoder.mask_features = Conv2d(64, 256, 3, padding=1) (fpn.py:237-246), the one
// trainable layer of the RGB-D configuration's pixel decoder.  Per tap this is a GEMM [Cout] x [64] whose reduction runs over EVERY
// pixel of the batch (K = B*H*W = 2.46 M at B = 8, 480 x 640; 725 GFLOP): MFMA work with a small result.
//
// The accumulator Cout x 576 does not fit a CU's registers, so a workgroup (four waves, one per SIMD) owns
//     one 64-channel slice of o  x  the three taps of one dy (64 x 192 accumulators = 192 registers per lane)  x  one range of pixels
// of the flattened pixel axis q = b*H*W + p (the `splits`; a range may cross image boundaries).  It walks its range in chunks of 64
// pixels, 16 per wave:
//   * g is pixel-contiguous per channel, x channel-contiguous per pixel: both go through LDS.  G[o][k] (row stride 72 floats: the
//     conflict-free ds_read_b128 stride of conv3x3.hip, 2 mod 4 slots) gives a lane the A operands of FOUR k-steps (pixels lq*4 .. +3 of
//     channel o = lj) in one read; X[k][c] (row stride 64: lanes = 16 slots of a row, the four rows of a read 256 floats apart, also
//     conflict-free) gives a lane the B operands of FOUR column blocks in one read: column j of block n is channel 4 j + n;
//   * v_mfma_f32_16x16x4_f32, D rows = output channels, columns = input channels, K = pixels: 64 MFMAs per (16 pixels, tap) on
//     4 + 4 LDS reads;
//   * the x rows of a chunk are the flattened pixels q + (dy-1)*W - 1 .. + 64: inside an image that is the tap's pixel; whether a tap
//     IS inside the image (the row y + dy - 1 and the column x + dx - 1: pixel (y, W-1) and pixel (y+1, 0) are neighbours in memory
//     only) is a 3-bit mask per pixel, computed once per chunk, and a masked B operand is an exact zero;
//   * the next chunk's global loads are issued before the current chunk's MFMAs and stored to LDS after them;
//   * the bias gradient comes from the g values a thread stages (dy = 1 workgroups only), reduced over the wave at the end.
// The four waves' tiles are added in LDS in wave order and written to the workspace [split][Cout][576] (+ [split][Cout] bias sums);
// a second kernel adds the splits in index order.  No atomics, no hand-off between workgroups: bit-identical from call to call.
#include "common.h"

namespace msm {

constexpr int WG_C = 64;                 // input channels
constexpr int WG_K = 9 * WG_C;           // 576
constexpr int WG_KP = 64;                // pixels per chunk: 16 per wave
constexpr int WG_LDG = WG_KP + 8;        // LDS row stride of the g tile (floats): 18 slots of 16 B
constexpr int WG_XR = WG_KP + 2;         // staged x pixels: the chunk and one neighbour on each side
constexpr int WG_LDT = 3 * WG_C + 4;     // LDS row stride of the result tile
constexpr int WG_T = 256;                // threads
constexpr int WG_GPT = WG_C * WG_KP / WG_T;                    // g values per thread and chunk: 16
constexpr int WG_XPT = (WG_XR * (WG_C / 4) + WG_T - 1) / WG_T;  // x float4 per thread and chunk: 5
constexpr int WG_MAX_SPLITS = 4096;

__global__ __launch_bounds__(WG_T) void conv3x3_c64_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                 float* __restrict__ ws, float* __restrict__ wsb, int H, int W, int Cout,
                                                                 int NP, int per) {
    // staging: G [64][WG_LDG], X [WG_XR][64], masks [64]; afterwards the result tile [64][WG_LDT]
    __shared__ __attribute__((aligned(16))) float sm[WG_C * WG_LDT];
    static_assert(WG_C * WG_LDG + WG_XR * WG_C + WG_KP <= WG_C * WG_LDT, "the staging buffers share the result tile's LDS");
    float* Gs = sm;
    float* Xs = sm + WG_C * WG_LDG;
    int* Ms = reinterpret_cast<int*>(Xs + WG_XR * WG_C);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lj = lane & 15, lq = lane >> 4;
    const int s = blockIdx.x, dy = blockIdx.y, o0 = (int)blockIdx.z * WG_C;
    const int HW = H * W;
    const int P0 = (int)min((int64_t)NP, (int64_t)s * per), P1 = (int)min((int64_t)NP, (int64_t)P0 + per);
    const int nchunks = (P1 - P0 + WG_KP - 1) / WG_KP;

    float gr[WG_GPT];
    float4 xr[WG_XPT];
    int mk = 0;
    // global loads of the chunk at pixel P into registers.  g: thread (row tid >> 6, pixel tid & 63), rows + 4 i; x: float4 tid + 256 i
    auto load_chunk = [&](int P) {
        const int q = P + lane;
        const bool ok = q < P1;
        const int qc = ok ? q : P1 - 1;
        const int b = qc / HW, p = qc - b * HW;
        const float* gp = g + ((int64_t)b * Cout + o0 + wave) * HW + p;
#pragma unroll
        for (int i = 0; i < WG_GPT; ++i) gr[i] = ok ? gp[(int64_t)i * 4 * HW] : 0.f;
        const int y = p / W, xx = p - y * W, yy = y + dy - 1;
        mk = (ok && yy >= 0 && yy < H) ? ((xx >= 1 ? 1 : 0) | 2 | (xx + 1 < W ? 4 : 0)) : 0;
        const int64_t x0 = (int64_t)P + (int64_t)(dy - 1) * W - 1;
#pragma unroll
        for (int i = 0; i < WG_XPT; ++i) {
            const int idx = tid + i * WG_T;
            const int64_t gq = x0 + (idx >> 4);
            const bool in = idx < WG_XR * (WG_C / 4) && gq >= 0 && gq < NP;
            const int64_t gc = min(max(gq, (int64_t)0), (int64_t)NP - 1);
            const float4 v = *reinterpret_cast<const float4*>(x + gc * WG_C + (idx & 15) * 4);
            xr[i] = in ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    float bs[WG_GPT];
#pragma unroll
    for (int i = 0; i < WG_GPT; ++i) bs[i] = 0.f;
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < WG_GPT; ++i) {
            Gs[(wave + 4 * i) * WG_LDG + lane] = gr[i];
            bs[i] += gr[i];
        }
        if (tid < WG_KP) Ms[tid] = mk;
#pragma unroll
        for (int i = 0; i < WG_XPT; ++i) {
            const int idx = tid + i * WG_T;
            if (idx < WG_XR * (WG_C / 4)) *reinterpret_cast<float4*>(Xs + idx * 4) = xr[i];
        }
    };

    f32x4 acc[4][3][4];          // [16-channel block of o][dx][column block n]: D row lq*4 + r = channel o, column lj = input channel 4 lj + n
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[mt][dx][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (nchunks > 0) load_chunk(P0);
    for (int ch = 0; ch < nchunks; ++ch) {
        store_chunk();
        __syncthreads();
        if (ch + 1 < nchunks) load_chunk(P0 + (ch + 1) * WG_KP);
        // this wave's 16 pixels: chunk pixels wave*16 + lq*4 + r, r = 0..3 = the four k-steps
        f32x4 a[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) a[mt] = *reinterpret_cast<const f32x4*>(Gs + (mt * 16 + lj) * WG_LDG + wave * 16 + lq * 4);
        const int4 m4 = *reinterpret_cast<const int4*>(Ms + wave * 16 + lq * 4);
        const int mr[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            f32x4 bx[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(Xs + (wave * 16 + lq * 4 + r + dx) * WG_C + lj * 4);
                bx[r] = ((mr[r] >> dx) & 1) ? v : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int n = 0; n < 4; ++n) acc[mt][dx][n] = mfma16(a[mt][r], bx[r][n], acc[mt][dx][n]);
        }
        __syncthreads();
    }

    // the four waves' tiles, added in wave order in LDS (the staging buffers are free: the loop ended on a barrier)
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float* tp = sm + (mt * 16 + lq * 4 + r) * WG_LDT + dx * WG_C + lj * 4;
                        f32x4 t = {acc[mt][dx][0][r], acc[mt][dx][1][r], acc[mt][dx][2][r], acc[mt][dx][3][r]};
                        if (w > 0) t = *reinterpret_cast<const f32x4*>(tp) + t;
                        *reinterpret_cast<f32x4*>(tp) = t;
                    }
        }
        __syncthreads();
    }
    float* wp = ws + ((int64_t)s * Cout + o0) * WG_K + dy * (3 * WG_C);
#pragma unroll
    for (int i = 0; i < WG_C * (3 * WG_C / 4) / WG_T; ++i) {
        const int idx = tid + i * WG_T;
        const int o = idx / (3 * WG_C / 4), c4 = idx - o * (3 * WG_C / 4);
        *reinterpret_cast<float4*>(wp + (int64_t)o * WG_K + c4 * 4) = *reinterpret_cast<const float4*>(sm + o * WG_LDT + c4 * 4);
    }
    if (dy == 1) {
#pragma unroll
        for (int i = 0; i < WG_GPT; ++i) {
            const float t = wave_sum(bs[i]);
            if (lane == 0) wsb[(int64_t)s * Cout + o0 + wave + 4 * i] = t;
        }
    }
}

// dw = the splits' tiles added in index order (n4 float4 each); dbias likewise from the bias sums
__global__ __launch_bounds__(256) void conv3x3_c64_wgrad_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ wsb,
                                                                       float* __restrict__ dw, float* __restrict__ db, int n4, int Cout, int S) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n4) {
        float4 t = reinterpret_cast<const float4*>(ws)[i];
        for (int s = 1; s < S; ++s) {
            const float4 v = reinterpret_cast<const float4*>(ws)[(int64_t)s * n4 + i];
            t.x += v.x, t.y += v.y, t.z += v.z, t.w += v.w;
        }
        reinterpret_cast<float4*>(dw)[i] = t;
    } else if (db && i - n4 < Cout) {
        const int o = i - n4;
        float t = wsb[o];
        for (int s = 1; s < S; ++s) t += wsb[(int64_t)s * Cout + o];
        db[o] = t;
    }
}

// the number of pixel ranges: the caller's, or by shape -- about two workgroups per CU over the 3 * Cout/64 (dy, slice) pairs, and
// never ranges shorter than four chunks
static int wgrad_splits(int64_t NP, int Cout, int splits) {
    if (splits > 0) return splits;
    const int pairs = 3 * (Cout / WG_C);
    const int64_t by_chip = max(1, 512 / pairs), by_work = max((int64_t)1, (NP + 4 * WG_KP - 1) / (4 * WG_KP));
    return (int)min(by_chip, by_work);
}

static bool wgrad_shape_ok(int B, int H, int W, int Cout, int splits) {
    return B > 0 && H > 0 && W > 0 && Cout > 0 && Cout % WG_C == 0 && Cout <= 1024 && splits >= 0 && splits <= WG_MAX_SPLITS &&
           (int64_t)B * H * W < ((int64_t)1 << 31) - 2 * WG_KP;
}

}  // namespace msm

using namespace msm;

extern "C" int64_t msm_conv3x3_c64_wgrad_workspace(int B, int H, int W, int Cout, int splits) {
    if (!wgrad_shape_ok(B, H, W, Cout, splits)) {
        set_error("msm_conv3x3_c64_wgrad_workspace: need B, H, W >= 1, Cout a multiple of 64 up to 1024 and 0 <= splits <= %d (B=%d H=%d W=%d Cout=%d splits=%d)",
                  WG_MAX_SPLITS, B, H, W, Cout, splits);
        return MSM_E_INVALID;
    }
    return (int64_t)wgrad_splits((int64_t)B * H * W, Cout, splits) * Cout * (WG_K + 1);
}

extern "C" int msm_conv3x3_c64_wgrad(const float* in_tokens, const float* gout_nchw, float* dw_tap_major, float* dbias, float* workspace,
                                     int B, int H, int W, int Cout, int splits, void* stream) {
    MSM_REQUIRE(in_tokens && gout_nchw && dw_tap_major && workspace, "msm_conv3x3_c64_wgrad: null pointer");
    MSM_REQUIRE(wgrad_shape_ok(B, H, W, Cout, splits),
                "msm_conv3x3_c64_wgrad: need B, H, W >= 1, Cout a multiple of 64 up to 1024 and 0 <= splits <= %d (B=%d H=%d W=%d Cout=%d splits=%d)",
                WG_MAX_SPLITS, B, H, W, Cout, splits);
    MSM_REQUIRE(((((uintptr_t)in_tokens) | ((uintptr_t)dw_tap_major) | ((uintptr_t)workspace)) & 15) == 0 &&
                    ((((uintptr_t)gout_nchw) | ((uintptr_t)dbias)) & 3) == 0,
                "msm_conv3x3_c64_wgrad: misaligned pointer");
    const int NP = B * H * W;
    const int S = wgrad_splits(NP, Cout, splits);
    const int per = cdiv(cdiv(NP, S), 16) * 16;          // pixels per range, whole 16-pixel groups
    float* wsb = workspace + (int64_t)S * Cout * WG_K;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(conv3x3_c64_wgrad_kernel, dim3(S, 3, Cout / WG_C), dim3(WG_T), 0, st, in_tokens, gout_nchw, workspace, wsb, H, W, Cout,
                       NP, per);
    MSM_CHECK_LAUNCH("msm_conv3x3_c64_wgrad");
    const int n4 = Cout * (WG_K / 4);
    hipLaunchKernelGGL(conv3x3_c64_wgrad_reduce_kernel, dim3(cdiv(n4 + Cout, 256)), dim3(256), 0, st, workspace, wsb, dw_tap_major, dbias, n4,
                       Cout, S);
    MSM_CHECK_LAUNCH("msm_conv3x3_c64_wgrad(reduce)");
    return MSM_OK;
}
