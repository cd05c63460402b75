// Raw camera frames -> the two NCHW fp32 tensors the network sees (the head of every entry point of the reference:
// tools/test_image_with_ms_transformer.py:115-147 read_sample, ros/test_images_segmentation_transformer.py:147-173
// run_network, compute_xyz lib/fcn/get_backbone.py:96-102).
//
// ONE launch for a batch of F frames; it also writes the zero border of a frame larger than the image (the padding of
// meta_arch._pad_to), so no memset launch precedes it.  Definition (every step fp32, round to nearest):
//   image[c][y][x] = lut[c][color[y][x][c']]           c' = c, or 2 - c with swap_rb; lut built by the host (frames.image_lut)
//   z              = float(d) / depth_div              uint16 depth;  float32 depth: z = d, NaN -> 0
//   xyz[0]         = ((float(x) - px) * z) / fx
//   xyz[1]         = ((float(y) - py) * z) / fy
//   xyz[2]         = z
//   rows y >= H and columns x >= W of the [Hp][Wp] frame: 0 in both tensors
// The image is a table lookup, so it is bit exact whatever the compiler does with a division; the xyz path is three
// correctly rounded operations with no multiply-add in it (written with the _rn intrinsics: no contraction, no
// reassociation, no reciprocal).
//
// A pure streaming kernel: 5 bytes per pixel read (3 colour + 2 depth), 24 written.  One lane takes FOUR consecutive pixels
// of a frame row: 12 colour bytes (three dwords), 8 / 16 depth bytes (one load), six 16-byte stores -- a wave writes 1 KiB of
// every output row segment per store instruction.  The two sides are vectorised independently:
//   VIN   W % 4 == 0 (every colour row starts on a dword, a quad lies inside or outside the image as a whole) and aligned bases
//   VOUT  Wp % 4 == 0 and 16-byte aligned outputs
// and fall back to element-wise loads / stores where that does not hold (same arithmetic, same values).
#include "common.h"

namespace {

constexpr int IG_THREADS = 256;

enum { IG_NO_DEPTH = 0, IG_U16 = 1, IG_F32 = 2 };

template <bool VIN, bool VOUT, int DK>
__global__ __launch_bounds__(IG_THREADS) void ingest_frames_kernel(const uint8_t* __restrict__ color, const void* __restrict__ depth,
                                                                   float depth_div, const float* __restrict__ lut,
                                                                   const float* __restrict__ cam, float* __restrict__ image_out,
                                                                   float* __restrict__ xyz_out, int H, int W, int Hp, int Wp, int Q,
                                                                   int64_t quads, int swap_rb) {
    __shared__ float tab[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += IG_THREADS) tab[i] = lut[i];
    __syncthreads();
    const int64_t plane = (int64_t)Hp * Wp;
    for (int64_t q = (int64_t)blockIdx.x * IG_THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * IG_THREADS) {
        const uint32_t row = (uint32_t)q / (uint32_t)Q;          // f * Hp + y (quads < 2^31: 32-bit divisions)
        const int x0 = (int)((uint32_t)q - row * (uint32_t)Q) * 4;
        const int f = (int)(row / (uint32_t)Hp), y = (int)(row - (uint32_t)f * (uint32_t)Hp);
        float im[3][4], xyz[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) im[c][i] = xyz[c][i] = 0.f;
        if (y < H && x0 < W) {
            const int64_t pix = ((int64_t)f * H + y) * W + x0;   // first input pixel of the quad
            uint8_t b[4][3];
            float z[4];
            bool in[4];
            if (VIN) {                                           // W % 4 == 0: the whole quad is inside
                const uint32_t* cp = reinterpret_cast<const uint32_t*>(color + pix * 3);
                const uint32_t w0 = cp[0], w1 = cp[1], w2 = cp[2];
#pragma unroll
                for (int k = 0; k < 12; ++k) {
                    const uint32_t w = k < 4 ? w0 : (k < 8 ? w1 : w2);
                    b[k / 3][k % 3] = (uint8_t)(w >> (8 * (k & 3)));
                }
                if (DK == IG_U16) {
                    const uint2 d = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(depth) + pix);
                    z[0] = (float)(d.x & 0xffffu); z[1] = (float)(d.x >> 16); z[2] = (float)(d.y & 0xffffu); z[3] = (float)(d.y >> 16);
                } else if (DK == IG_F32) {
                    const float4 d = *reinterpret_cast<const float4*>(static_cast<const float*>(depth) + pix);
                    z[0] = d.x; z[1] = d.y; z[2] = d.z; z[3] = d.w;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) in[i] = true;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    in[i] = x0 + i < W;
                    z[i] = 0.f;
                    b[i][0] = b[i][1] = b[i][2] = 0;
                    if (in[i]) {
                        const uint8_t* cp = color + (pix + i) * 3;
                        b[i][0] = cp[0]; b[i][1] = cp[1]; b[i][2] = cp[2];
                        if (DK == IG_U16) z[i] = (float)static_cast<const uint16_t*>(depth)[pix + i];
                        if (DK == IG_F32) z[i] = static_cast<const float*>(depth)[pix + i];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (in[i]) {
                    im[0][i] = tab[swap_rb ? b[i][2] : b[i][0]];           // output channel c reads input channel 2 - c
                    im[1][i] = tab[256 + b[i][1]];
                    im[2][i] = tab[512 + (swap_rb ? b[i][0] : b[i][2])];
                }
            }
            if (DK != IG_NO_DEPTH) {
                const float fx = cam[f * 4 + 0], fy = cam[f * 4 + 1], px = cam[f * 4 + 2], py = cam[f * 4 + 3];
                const float yc = __fsub_rn((float)y, py);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (in[i]) {
                        float zi = z[i];
                        if (DK == IG_U16) zi = __fdiv_rn(zi, depth_div);
                        if (DK == IG_F32) zi = zi != zi ? 0.f : zi;                       // NaN -> 0 (run_network:170)
                        xyz[0][i] = __fdiv_rn(__fmul_rn(__fsub_rn((float)(x0 + i), px), zi), fx);
                        xyz[1][i] = __fdiv_rn(__fmul_rn(yc, zi), fy);
                        xyz[2][i] = zi;
                    }
                }
            }
        }
        const int64_t o = (int64_t)f * 3 * plane + (int64_t)y * Wp + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (VOUT) {                                          // Wp % 4 == 0: the quad lies inside the frame row
                *reinterpret_cast<float4*>(image_out + o + c * plane) = make_float4(im[c][0], im[c][1], im[c][2], im[c][3]);
                if (DK != IG_NO_DEPTH)
                    *reinterpret_cast<float4*>(xyz_out + o + c * plane) = make_float4(xyz[c][0], xyz[c][1], xyz[c][2], xyz[c][3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (x0 + i < Wp) {
                        image_out[o + c * plane + i] = im[c][i];
                        if (DK != IG_NO_DEPTH) xyz_out[o + c * plane + i] = xyz[c][i];
                    }
                }
            }
        }
    }
}

template <bool VIN, bool VOUT>
void launch(int dk, int grid, hipStream_t s, const uint8_t* color, const void* depth, float depth_div, const float* lut, const float* cam,
            float* image_out, float* xyz_out, int H, int W, int Hp, int Wp, int Q, int64_t quads, int swap_rb) {
    if (dk == IG_U16)
        hipLaunchKernelGGL((ingest_frames_kernel<VIN, VOUT, IG_U16>), dim3(grid), dim3(IG_THREADS), 0, s, color, depth, depth_div, lut, cam,
                           image_out, xyz_out, H, W, Hp, Wp, Q, quads, swap_rb);
    else if (dk == IG_F32)
        hipLaunchKernelGGL((ingest_frames_kernel<VIN, VOUT, IG_F32>), dim3(grid), dim3(IG_THREADS), 0, s, color, depth, depth_div, lut, cam,
                           image_out, xyz_out, H, W, Hp, Wp, Q, quads, swap_rb);
    else
        hipLaunchKernelGGL((ingest_frames_kernel<VIN, VOUT, IG_NO_DEPTH>), dim3(grid), dim3(IG_THREADS), 0, s, color, depth, depth_div, lut, cam,
                           image_out, xyz_out, H, W, Hp, Wp, Q, quads, swap_rb);
}

}  // namespace

extern "C" int msm_ingest_frames(const uint8_t* color, const void* depth, int depth_is_u16, float depth_div, const float* lut,
                                 const float* cam, float* image_out, float* xyz_out, int F, int H, int W, int Hp, int Wp,
                                 int swap_rb, void* stream) {
    MSM_REQUIRE(color && lut && image_out, "msm_ingest_frames: null pointer (color, lut and image_out are required)");
    MSM_REQUIRE((depth == nullptr) == (xyz_out == nullptr), "msm_ingest_frames: depth and xyz_out go together");
    MSM_REQUIRE(depth == nullptr || cam != nullptr, "msm_ingest_frames: depth needs the intrinsics table cam");
    MSM_REQUIRE(F >= 0 && H > 0 && W > 0, "msm_ingest_frames: bad shape F=%d H=%d W=%d", F, H, W);
    MSM_REQUIRE(Hp >= H && Wp >= W, "msm_ingest_frames: the frame %dx%d is smaller than the image %dx%d", Hp, Wp, H, W);
    MSM_REQUIRE(depth_div > 0.f, "msm_ingest_frames: depth_div must be positive");
    MSM_REQUIRE((((uintptr_t)lut | (uintptr_t)cam | (uintptr_t)image_out | (uintptr_t)xyz_out) & 3) == 0 &&
                    ((uintptr_t)depth & (depth_is_u16 ? 1 : 3)) == 0,
                "msm_ingest_frames: misaligned pointer");
    if (F == 0) return MSM_OK;
    const int Q = msm::cdiv(Wp, 4);
    const int64_t quads = (int64_t)F * Hp * Q;
    MSM_REQUIRE(quads < ((int64_t)1 << 31), "msm_ingest_frames: %d frames of %dx%d are too many for one launch", F, Hp, Wp);
    const int dk = depth == nullptr ? IG_NO_DEPTH : (depth_is_u16 ? IG_U16 : IG_F32);
    const bool vin = W % 4 == 0 && ((uintptr_t)color & 3) == 0 && ((uintptr_t)depth & (depth_is_u16 ? 7 : 15)) == 0;
    const bool vout = Wp % 4 == 0 && (((uintptr_t)image_out | (uintptr_t)xyz_out) & 15) == 0;
    const int grid = (int)max((int64_t)1, min((quads + IG_THREADS - 1) / IG_THREADS, (int64_t)2048));
    hipStream_t s = (hipStream_t)stream;
    if (vin && vout) launch<true, true>(dk, grid, s, color, depth, depth_div, lut, cam, image_out, xyz_out, H, W, Hp, Wp, Q, quads, swap_rb);
    else if (vin) launch<true, false>(dk, grid, s, color, depth, depth_div, lut, cam, image_out, xyz_out, H, W, Hp, Wp, Q, quads, swap_rb);
    else if (vout) launch<false, true>(dk, grid, s, color, depth, depth_div, lut, cam, image_out, xyz_out, H, W, Hp, Wp, Q, quads, swap_rb);
    else launch<false, false>(dk, grid, s, color, depth, depth_div, lut, cam, image_out, xyz_out, H, W, Hp, Wp, Q, quads, swap_rb);
    MSM_CHECK_LAUNCH("msm_ingest_frames");
    return MSM_OK;
}
