// What a meta-arch applies to a batch in front of the network, in ONE launch: (x - pixel_mean) / pixel_std on the image
// (meanshiftformer_model.py:241-242), then the zero padding of image and depth to the size divisibility
// (ImageList.from_tensors).  In torch that is three launches and three passes (sub, div, F.pad).
//
// Definition (every step fp32, round to nearest; written with the _rn intrinsics like the xyz path of ingest.hip: no
// reciprocal, no multiply-add):
//   image_out[n][c][y][x] = (image[n][c][y][x] - mean[c]) / std[c]        y < H, x < W; without mean: the same bits
//   depth_out[n][c][y][x] = depth[n][c][y][x]                             the same bits (NaN payloads included)
//   rows y >= H and columns x >= W of the [Hp][Wp] frames: +0.0 in both outputs, written by this launch (no memset in front)
//
// A pure streaming kernel: 4 bytes read and 4 written per element.  The N (C + Cd) planes of both tensors are one index space;
// one lane takes FOUR consecutive elements of an output row.  The two sides are vectorised independently, as in ingest.hip:
//   VIN   W % 4 == 0 and 16-byte aligned inputs (a quad lies inside or outside the image as a whole)
//   VOUT  Wp % 4 == 0 and 16-byte aligned outputs
// and fall back to element-wise loads / stores where that does not hold (same arithmetic, same values).  Values travel as
// 32-bit words, so a copy cannot touch a NaN's payload.
#include "common.h"

namespace {

constexpr int PP_THREADS = 256;

template <bool VIN, bool VOUT>
__global__ __launch_bounds__(PP_THREADS) void prepare_inputs_kernel(const uint32_t* __restrict__ image, const uint32_t* __restrict__ depth,
                                                                    const float* __restrict__ mean, const float* __restrict__ stdv,
                                                                    uint32_t* __restrict__ image_out, uint32_t* __restrict__ depth_out,
                                                                    int C, int Cd, int H, int W, int Hp, int Wp, int Q, int64_t quads) {
    const uint32_t CC = (uint32_t)(C + Cd);
    for (int64_t q = (int64_t)blockIdx.x * PP_THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * PP_THREADS) {
        const uint32_t row = (uint32_t)q / (uint32_t)Q;          // plane * Hp + y (quads < 2^31: 32-bit divisions)
        const int x0 = (int)((uint32_t)q - row * (uint32_t)Q) * 4;
        const uint32_t p = row / (uint32_t)Hp;                   // plane n * (C + Cd) + ch
        const int y = (int)(row - p * (uint32_t)Hp);
        const uint32_t n = p / CC;
        const int ch = (int)(p - n * CC);
        const bool is_image = ch < C;
        const int c = is_image ? ch : ch - C;                    // channel inside its own tensor
        const int64_t pl = is_image ? (int64_t)n * C + c : (int64_t)n * Cd + c;
        const uint32_t* __restrict__ src = (is_image ? image : depth) + pl * ((int64_t)H * W);
        uint32_t* __restrict__ dst = (is_image ? image_out : depth_out) + pl * ((int64_t)Hp * Wp) + (int64_t)y * Wp + x0;
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        if (y < H && x0 < W) {
            const uint32_t* __restrict__ sp = src + (int64_t)y * W + x0;
            bool in[4];
            if (VIN) {                                           // W % 4 == 0: the whole quad is inside
                const uint4 t = *reinterpret_cast<const uint4*>(sp);
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
#pragma unroll
                for (int i = 0; i < 4; ++i) in[i] = true;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    in[i] = x0 + i < W;
                    if (in[i]) v[i] = sp[i];
                }
            }
            if (is_image && mean != nullptr) {
                const float m = mean[c], s = stdv[c];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (in[i]) v[i] = __float_as_uint(__fdiv_rn(__fsub_rn(__uint_as_float(v[i]), m), s));
            }
        }
        if (VOUT) {                                              // Wp % 4 == 0: the quad lies inside the frame row
            *reinterpret_cast<uint4*>(dst) = make_uint4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x0 + i < Wp) dst[i] = v[i];
        }
    }
}

}  // namespace

extern "C" int msm_prepare_inputs(const float* image, const float* depth, const float* mean, const float* stdv, float* image_out,
                                  float* depth_out, int N, int C, int Cd, int H, int W, int Hp, int Wp, void* stream) {
    MSM_REQUIRE(image && image_out, "msm_prepare_inputs: null pointer (image and image_out are required)");
    MSM_REQUIRE((depth == nullptr) == (depth_out == nullptr), "msm_prepare_inputs: depth and depth_out go together");
    MSM_REQUIRE((depth == nullptr) == (Cd == 0), "msm_prepare_inputs: Cd = %d %s depth", Cd, depth ? "with" : "without");
    MSM_REQUIRE((mean == nullptr) == (stdv == nullptr), "msm_prepare_inputs: mean and std go together");
    MSM_REQUIRE(N >= 0 && C > 0 && Cd >= 0 && H > 0 && W > 0, "msm_prepare_inputs: bad shape N=%d C=%d Cd=%d H=%d W=%d", N, C, Cd, H, W);
    MSM_REQUIRE(Hp >= H && Wp >= W, "msm_prepare_inputs: the frame %dx%d is smaller than the image %dx%d", Hp, Wp, H, W);
    MSM_REQUIRE((((uintptr_t)image | (uintptr_t)depth | (uintptr_t)mean | (uintptr_t)stdv | (uintptr_t)image_out | (uintptr_t)depth_out) & 3) == 0,
                "msm_prepare_inputs: misaligned pointer");
    MSM_REQUIRE(image != image_out && (depth == nullptr || depth != depth_out), "msm_prepare_inputs: an output is its own input (there is no in-place form)");
    if (N == 0) return MSM_OK;
    const int Q = msm::cdiv(Wp, 4);
    const int64_t quads = (int64_t)N * (C + Cd) * Hp * Q;
    MSM_REQUIRE(quads < ((int64_t)1 << 31), "msm_prepare_inputs: %d x %d planes of %dx%d are too many for one launch", N, C + Cd, Hp, Wp);
    const bool vin = W % 4 == 0 && (((uintptr_t)image | (uintptr_t)depth) & 15) == 0;
    const bool vout = Wp % 4 == 0 && (((uintptr_t)image_out | (uintptr_t)depth_out) & 15) == 0;
    const int grid = (int)max((int64_t)1, min((quads + PP_THREADS - 1) / PP_THREADS, (int64_t)2048));
    hipStream_t s = (hipStream_t)stream;
    const uint32_t* im = reinterpret_cast<const uint32_t*>(image);
    const uint32_t* dp = reinterpret_cast<const uint32_t*>(depth);
    uint32_t* imo = reinterpret_cast<uint32_t*>(image_out);
    uint32_t* dpo = reinterpret_cast<uint32_t*>(depth_out);
#define PP_LAUNCH(VI, VO) \
    hipLaunchKernelGGL((prepare_inputs_kernel<VI, VO>), dim3(grid), dim3(PP_THREADS), 0, s, im, dp, mean, stdv, imo, dpo, C, Cd, H, W, Hp, Wp, Q, quads)
    if (vin && vout) PP_LAUNCH(true, true);
    else if (vin) PP_LAUNCH(true, false);
    else if (vout) PP_LAUNCH(false, true);
    else PP_LAUNCH(false, false);
#undef PP_LAUNCH
    MSM_CHECK_LAUNCH("msm_prepare_inputs");
    return MSM_OK;
}
