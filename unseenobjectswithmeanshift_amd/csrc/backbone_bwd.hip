// Backward of the UCN embedding tail (csrc/backbone_ops.hip, ucn_tail_kernel): training the RGB-D backbone from images.
//
//   forward    u = up(a) + up(b2),  y = N^norms(u),  N(v) = v / max(|v|_2, eps) over the 64 channels,  up = bilinear, align_corners=True
//   backward   g_u = dN(u)^T .. dN(y_1)^T g,  gin = up^T g_u   (add fusion: the gradient of a and of b2 is the same tensor)
//   dN(v)^T g  = (g - y <y, g>) / |v|  with y = v / |v|     where |v| >= eps
//              = g / eps                                    where |v| <  eps   (torch: clamp_min passes no gradient to the norm below eps)
//
// The specification is torch's float64 autograd of F.interpolate(bilinear, align_corners=True), +, F.normalize(p=2, dim=1, eps) x norms.
//
// Form: a two-stage reduction in fixed order, no atomics -- the bilinear adjoint is separable, up^T = Uy^T (.) Ux^T.
//   stage 1 (ucn_tail_bwd_rows_kernel)  one workgroup per (image, output row Y, tile of TJ low-resolution columns): it walks the output pixels
//            of the row whose x taps reach the tile in chunks of 64, recomputes u from the low-resolution maps with the forward's tap
//            indices and weights (the row's two source rows are blended once per workgroup in LDS; y is never read), reads the pixel's 64
//            gradients ONCE, forms g_u, and sums it over x in LDS in increasing x:  T[b][Y][j][c] = sum_X wx(X, j) g_u[b][c][Y][X]
//   stage 2 (ucn_tail_bwd_cols_kernel)  gin[b][i][j][c] = sum_Y wy(Y, i) T[b][Y][j][c] in increasing Y, sixteen bytes per thread.
// Traffic: gout once (plus the halo of one low-resolution column per tile: 1 / TJ more at x8), the low-resolution maps, T written once
// and read twice (every row feeds two low-resolution rows), T = 1 / (W / w) of gout; a full-size g_u never exists in memory.
// Tap geometry is the forward's, in fp32: sx = rx * (float)x, x0 = (int)sx, x1 = x0 + (x0 < w - 1); the set of output pixels that reach a
// low-resolution column is found from that same expression (it is monotone in x) by bisection, so downsampling, single rows / columns
// and the identity size need no case of their own.
#include "common.h"

namespace msm {

// low-resolution columns per workgroup of stage 1 (at most 16: the sum phase has 16 column slots of 16 threads).  At the backbone's x8 the
// pixels that reach 15 columns are 15 * 8 + 8 = 128: two full chunks
constexpr int TB_TJ = 15;

// the smallest X in [0, N] with min((int)(r * (float)X), n - 1) >= t (N when there is none): the forward's own source index, monotone in X
__device__ __forceinline__ int first_reaching(float r, int n, int N, int t) {
    int lo = 0, hi = N;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (min((int)(r * (float)mid), n - 1) >= t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// Block: 256 threads.  Compute phase: thread (px = tid & 63, cq = tid >> 6) owns channels 16 cq .. + 15 of pixel X = chunk + px, as the
// forward.  Sum phase: thread (sc = tid & 15, sm = tid >> 4) owns channels 4 sc .. + 3 of column j0 + sm.
__global__ __launch_bounds__(256, 4) void ucn_tail_bwd_rows_kernel(const float* __restrict__ a, const float* __restrict__ b2, const float* __restrict__ gout,
                                                                float* __restrict__ T, int h, int w, int H, int W, float ry, float rx, int norms,
                                                                float eps) {
    __shared__ __attribute__((aligned(16))) float gu[64][68];   // g_u of the chunk, [px][c]; rows of 17 x 16 bytes: 16-byte LDS accesses in both phases
    __shared__ __attribute__((aligned(16))) float mix[TB_TJ + 2][68];   // the low-resolution columns j0 - 1 .. j0 + TJ, interpolated in y
    __shared__ float red[3][4][64];         // the channel reductions of a pixel: [which][cq][px]
    __shared__ float s_hx[64], s_lx[64];    // the x weights of the chunk's pixels
    __shared__ int s_first[TB_TJ + 2];      // s_first[m] = first X whose x0 >= j0 - 1 + m
    const int tid = threadIdx.x;
    const int px = tid & 63, cq = tid >> 6;
    const int sc = tid & 15, sm = tid >> 4;
    const int j0 = blockIdx.x * TB_TJ, Y = blockIdx.y, b = blockIdx.z;
    if (tid < TB_TJ + 2) s_first[tid] = first_reaching(rx, w, W, j0 - 1 + tid);
    const float sy = ry * (float)Y;
    const int y0 = min((int)sy, h - 1);
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0);
    const float ly = sy - (float)y0, hy = 1.f - ly;
    if (norms > 0) {
        // the row is fixed, so the y half of the interpolation is done once per workgroup: mix[col] = hy (a + b2)[y0][x] + ly (a + b2)[y1][x]
        // for the columns x = j0 - 1 + col the row's pixels can tap; u = hx mix[x0] + lx mix[x1] then costs two LDS reads per pixel instead
        // of eight cache reads (up(a) + up(b2) = up(a + b2), the tap indices and weights are the forward's)
        for (int e = tid; e < (TB_TJ + 2) * 16; e += 256) {
            const int col = e >> 4, x = j0 - 1 + col;
            if (x < 0 || x >= w) continue;
            const int64_t o0 = (((int64_t)b * h + y0) * w + x) * 64 + (e & 15) * 4, o1 = (((int64_t)b * h + y1) * w + x) * 64 + (e & 15) * 4;
            float4 q0 = *reinterpret_cast<const float4*>(a + o0), q1 = *reinterpret_cast<const float4*>(a + o1);
            if (b2 != nullptr) {
                const float4 t0 = *reinterpret_cast<const float4*>(b2 + o0), t1 = *reinterpret_cast<const float4*>(b2 + o1);
                q0.x += t0.x, q0.y += t0.y, q0.z += t0.z, q0.w += t0.w;
                q1.x += t1.x, q1.y += t1.y, q1.z += t1.z, q1.w += t1.w;
            }
            *reinterpret_cast<float4*>(&mix[col][(e & 15) * 4]) =
                make_float4(hy * q0.x + ly * q1.x, hy * q0.y + ly * q1.y, hy * q0.z + ly * q1.z, hy * q0.w + ly * q1.w);
        }
    }
    __syncthreads();
    // the output pixels whose taps reach columns j0 .. j0 + TJ - 1: x0 in [j0 - 1, j0 + TJ - 1]
    const int Xlo = s_first[0], Xhi = s_first[TB_TJ + 1];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int chunk = Xlo; chunk < Xhi; chunk += 64) {
        const int X = chunk + px;
        const bool live = X < Xhi;
        const float sx = rx * (float)min(X, W - 1);
        const int x0 = min((int)sx, w - 1);
        const int x1 = x0 + (x0 < w - 1 ? 1 : 0);
        const float lx = sx - (float)x0, hx = 1.f - lx;
        float u[16], g[16];
        if (norms > 0) {
            // (a pixel past the range is not summed; its taps are clamped into the staged columns)
            const float* r0 = mix[min(max(x0 - j0 + 1, 0), TB_TJ + 1)] + cq * 16;
            const float* r1 = mix[min(max(x1 - j0 + 1, 0), TB_TJ + 1)] + cq * 16;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 q0 = reinterpret_cast<const float4*>(r0)[k], q1 = reinterpret_cast<const float4*>(r1)[k];
                u[4 * k + 0] = hx * q0.x + lx * q1.x, u[4 * k + 1] = hx * q0.y + lx * q1.y;
                u[4 * k + 2] = hx * q0.z + lx * q1.z, u[4 * k + 3] = hx * q0.w + lx * q1.w;
            }
        }
        {
            const float* gp = gout + (((int64_t)b * 64 + cq * 16) * H + Y) * W + min(X, W - 1);
#pragma unroll
            for (int i = 0; i < 16; ++i) g[i] = live ? gp[(int64_t)i * H * W] : 0.f;
        }
        if (norms > 0) {
            // forward: y1 = u / max(n1, eps), y2 = y1 / max(n2, eps); backward in the reverse order.  <u, u> and <u, g> share one
            // barrier: <y1, g> = <u, g> / max(n1, eps), |y1| = n1 / max(n1, eps), <y2, g> = <y1, g> / max(n2, eps)
            float puu = 0.f, pug = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) puu += u[i] * u[i], pug += u[i] * g[i];
            red[0][cq][px] = puu, red[1][cq][px] = pug;
            __syncthreads();
            const float n1 = sqrtf((red[0][0][px] + red[0][1][px]) + (red[0][2][px] + red[0][3][px]));
            const float inv1 = 1.f / fmaxf(n1, eps);
            float dot = ((red[1][0][px] + red[1][1][px]) + (red[1][2][px] + red[1][3][px])) * inv1;      // <y1, g>
#pragma unroll
            for (int i = 0; i < 16; ++i) u[i] *= inv1;                       // u is y1 from here on
            if (norms > 1) {
                const float n2 = n1 * inv1;
                const float inv2 = 1.f / fmaxf(n2, eps);
                const float dot2 = n2 >= eps ? dot * inv2 : 0.f;             // <y2, g>
                float part = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    g[i] = (g[i] - (u[i] * inv2) * dot2) * inv2;             // the gradient of y1
                    part += u[i] * g[i];
                }
                red[2][cq][px] = part;
                __syncthreads();
                dot = (red[2][0][px] + red[2][1][px]) + (red[2][2][px] + red[2][3][px]);
            }
            const float dot1 = n1 >= eps ? dot : 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) g[i] = (g[i] - u[i] * dot1) * inv1;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            *reinterpret_cast<float4*>(&gu[px][cq * 16 + 4 * k]) = make_float4(g[4 * k], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3]);
        if (cq == 0) s_hx[px] = hx + (x1 == x0 ? lx : 0.f), s_lx[px] = lx;   // at the last column both taps are the same pixel
        __syncthreads();
        // sum phase, in increasing X: column j takes lx g_u from the pixels with x0 == j - 1 (their x1 is j) and hx g_u from those with x0 == j
        if (sm < TB_TJ) {
            const int a0 = max(s_first[sm], chunk), a1 = min(s_first[sm + 1], chunk + 64);
            const int b0 = max(s_first[sm + 1], chunk), b1 = min(s_first[sm + 2], chunk + 64);
            for (int p = a0 - chunk; p < a1 - chunk; ++p) {
                const float wgt = s_lx[p];
                const float4 t = *reinterpret_cast<const float4*>(&gu[p][sc * 4]);
                acc.x += wgt * t.x, acc.y += wgt * t.y, acc.z += wgt * t.z, acc.w += wgt * t.w;
            }
            for (int p = b0 - chunk; p < b1 - chunk; ++p) {
                const float wgt = s_hx[p];
                const float4 t = *reinterpret_cast<const float4*>(&gu[p][sc * 4]);
                acc.x += wgt * t.x, acc.y += wgt * t.y, acc.z += wgt * t.z, acc.w += wgt * t.w;
            }
        }
        __syncthreads();                                                     // gu and the weights are rewritten by the next chunk
    }
    if (sm < TB_TJ && j0 + sm < w) *reinterpret_cast<float4*>(T + (((int64_t)b * H + Y) * w + j0 + sm) * 64 + sc * 4) = acc;
}

// gin[b][i][j][c .. c + 3] = sum over the rows Y that reach i of wy(Y, i) T[b][Y][j][c .. c + 3], in increasing Y
__global__ __launch_bounds__(256) void ucn_tail_bwd_cols_kernel(const float* __restrict__ T, float* __restrict__ gin, int64_t total, int h, int w, int H,
                                                                float ry) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;             // (b, i, j, c / 4)
    if (idx >= total) return;
    const int c4 = (int)(idx & 15);
    const int64_t pix = idx >> 4;
    const int j = (int)(pix % w);
    const int i = (int)((pix / w) % h);
    const int64_t b = pix / ((int64_t)w * h);
    const int Y0 = first_reaching(ry, h, H, i - 1), Y1 = first_reaching(ry, h, H, i + 1);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* base = T + ((b * H) * w + j) * 64 + c4 * 4;
    for (int Y = Y0; Y < Y1; ++Y) {
        const float sy = ry * (float)Y;
        const int y0 = min((int)sy, h - 1);
        const int y1 = y0 + (y0 < h - 1 ? 1 : 0);
        const float ly = sy - (float)y0, hy = 1.f - ly;
        const float wgt = (y0 == i ? hy : 0.f) + (y1 == i ? ly : 0.f);
        const float4 t = *reinterpret_cast<const float4*>(base + (int64_t)Y * w * 64);
        acc.x += wgt * t.x, acc.y += wgt * t.y, acc.z += wgt * t.z, acc.w += wgt * t.w;
    }
    reinterpret_cast<float4*>(gin)[idx] = acc;
}

}  // namespace msm

using namespace msm;

extern "C" int64_t msm_ucn_embedding_tail_bwd_workspace(int B, int H, int w) {
    if (B <= 0 || H <= 0 || w <= 0) {
        set_error("msm_ucn_embedding_tail_bwd_workspace: need B, H, w >= 1 (B=%d H=%d w=%d)", B, H, w);
        return MSM_E_INVALID;
    }
    return (int64_t)B * H * w * 64;
}

extern "C" int msm_ucn_embedding_tail_bwd(const float* a, const float* b2, const float* gout, float* gin, float* workspace, int64_t workspace_floats,
                                          int B, int h, int w, int H, int W, int norms, float eps, void* stream) {
    const char* who = "msm_ucn_embedding_tail_bwd";
    MSM_REQUIRE(a && gout && gin && workspace && B > 0 && B <= 65535 && h > 0 && w > 0 && H > 0 && H <= 65535 && W > 0, "%s: bad arguments", who);
    MSM_REQUIRE(norms >= 0 && norms <= 2, "%s: norms=%d (0, 1 or 2 normalisations)", who, norms);
    MSM_REQUIRE(((((uintptr_t)a) | ((uintptr_t)b2) | ((uintptr_t)gin) | ((uintptr_t)workspace)) & 15) == 0 && (((uintptr_t)gout) & 3) == 0,
                "%s: the low-resolution maps and the workspace must be 16-byte aligned", who);
    if (workspace_floats < (int64_t)B * H * w * 64) {
        set_error("%s: workspace of %lld floats, %lld needed", who, (long long)workspace_floats, (long long)B * H * w * 64);
        return MSM_E_WORKSPACE;
    }
    const int64_t total = (int64_t)B * h * w * 16;
    MSM_REQUIRE((total + 255) / 256 <= 0x7fffffffLL, "%s: B*h*w=%lld too large", who, (long long)(total / 16));
    const float ry = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, rx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    hipLaunchKernelGGL(ucn_tail_bwd_rows_kernel, dim3(cdiv(w, TB_TJ), H, B), dim3(256), 0, (hipStream_t)stream, a, b2, gout, workspace, h, w, H, W, ry,
                       rx, norms, eps);
    MSM_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(ucn_tail_bwd_cols_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, workspace, gin, total, h, w, H,
                       ry);
    MSM_CHECK_LAUNCH(who);
    return MSM_OK;
}
