// Training crops (TRAIN.SYN_CROP): TableTopDataset.pad_crop_resize lib/datasets/tabletop_dataset.py:234-300,354-358 for a whole
// batch on the device -- one object per frame, its box squared, padded and clamped (msm_crop_boxes), then the colour frame, the
// label image and the ordered point cloud cropped there and resized to S x S (msm_train_crop).  The definitions C1-C4 are in
// msm_hip.h and, a second time, in the numpy host path of crops.py; every value is an integer or an exact float64, the results
// do not depend on which lane computes what.
//
//   msm_crop_boxes   one lane per image: a few words of the image's target table, some float64 arithmetic, two 16-byte stores.
//   msm_train_crop   a gather of B S^2 pixels without arithmetic intensity: what matters is that the stores are whole and the
//                    loads of a wave stay inside a few source rows.  A workgroup takes a band of 8 output rows of one image;
//                    the S column records (two taps, weight, nearest index: one int4 each, one ds_read_b128 per pixel) are
//                    computed once per workgroup into LDS, a wave takes one output row at a time (its row record is
//                    wave-uniform), a lane four consecutive output pixels: the wave reads two source rows (colour), one
//                    (label, xyz) and stores 768 contiguous bytes of colour, 1 KiB of each xyz plane.
// Every index taken from a box or a table is bounded before it is used; every loop is counted.
#include "common.h"

namespace {

constexpr int TG_BINS = MSM_TARGET_BINS;
constexpr int TG_MAXI = TG_BINS - 1;
constexpr int TG_INST = 4 + 2 * TG_BINS;               // the instance records of a target table row (csrc/targets.hip)
constexpr int TG_ROW = TG_INST + TG_MAXI * 6;
static_assert(TG_ROW == MSM_TARGET_TABLE_ROW, "msm_hip.h documents the table row");
constexpr int CB_ROW = MSM_CROP_BOX_ROW;
static_assert(CB_ROW == 8, "a box row is two 16-byte stores");
constexpr int CB_THREADS = 64;
constexpr int TC_THREADS = 256;
constexpr int TC_BAND = 8;                             // output rows per workgroup: two per wave
constexpr int TC_MAXS = MSM_CROP_MAX_SIZE;
constexpr int TC_WBITS = 11, TC_WONE = 1 << TC_WBITS;  // C4: weights in 1 / 2048

__global__ __launch_bounds__(CB_THREADS) void crop_boxes_kernel(const int32_t* __restrict__ tables, const int32_t* __restrict__ params,
                                                                int32_t* __restrict__ boxes, int B, int H, int W) {
    const int b = blockIdx.x * CB_THREADS + threadIdx.x;
    if (b >= B) return;
    const int32_t* tab = tables + (int64_t)b * TG_ROW;
    const int Tb = tab[1], Kb = tab[2];
    const uint32_t key = (uint32_t)params[2 * b];
    const float p = __int_as_float(params[2 * b + 1]);
    int status = (p >= 0.f && p <= 16.f) ? 0 : MSM_CROP_BAD_ROW;               // false for a NaN
    int idx = 0, id = -1, padding = 0;
    int bx0 = 0, by0 = 0, bx1 = W - 1, by1 = H - 1;                            // C1: the region's tight box
    const int64_t K = (int64_t)Kb - 1;                                         // 64 bits: a table that contradicts itself must not overflow
    if (!status && K > 0) {
        const int pick = 1 + (int)(((uint64_t)key * (uint64_t)K) >> 32);
        const int64_t t = (int64_t)pick - ((int64_t)Kb - (int64_t)Tb);
        bool ok = t >= 0 && t < Tb && t < TG_MAXI;
        int r[6] = {0, 0, 0, 0, 0, 0};
        if (ok) {
#pragma unroll
            for (int j = 0; j < 6; ++j) r[j] = tab[TG_INST + t * 6 + j];
            ok = r[2] >= 0 && r[2] <= r[4] && r[4] <= W - 1 && r[3] >= 0 && r[3] <= r[5] && r[5] <= H - 1;
        }
        if (ok) {
            idx = pick; id = r[0];
            bx0 = r[2]; by0 = r[3]; bx1 = r[4]; by1 = r[5];
        } else {
            status = MSM_CROP_BAD_ROW;
        }
    }
    int x0 = 0, y0 = 0, x1 = W - 1, y1 = H - 1;
    if (!status) {                                                             // C2, float64 in the reference's order
        double x_min = (double)bx0, y_min = (double)by0, x_max = (double)bx1, y_max = (double)by1;
        const double cx = (x_min + x_max) / 2.0, cy = (y_min + y_max) / 2.0;
        const double x_delta = x_max - x_min, y_delta = y_max - y_min;
        if (x_delta > y_delta) {
            y_min = cy - x_delta / 2.0;
            y_max = cy + x_delta / 2.0;
        } else {
            x_min = cx - y_delta / 2.0;
            x_max = cx + y_delta / 2.0;
        }
        const double side = x_max - x_min;
        padding = (int)rint(side * (double)p);                                 // the one rounded product; ties to even
        if (padding == 0) padding = 25;
        const double pd = (double)padding;
        x0 = max((int)(x_min - pd), 0);                                        // a cast truncates toward zero, as int() does
        x1 = min((int)(x_max + pd), W - 1);
        y0 = max((int)(y_min - pd), 0);
        y1 = min((int)(y_max + pd), H - 1);
        if (!(x0 < x1 && y0 < y1)) {                                           // cannot happen with H, W >= 2
            status = MSM_CROP_DEGENERATE;
            x0 = 0; y0 = 0; x1 = W - 1; y1 = H - 1;
        }
    }
    int4* row = reinterpret_cast<int4*>(boxes + (int64_t)b * CB_ROW);
    row[0] = make_int4(x0, y0, x1, y1);
    row[1] = make_int4(idx, id, padding, status);
}

// the record of output index d along an axis with source extent n: x = first tap, y = second tap, z = weight of the second tap
// (C4), w = nearest source index (C3)
__device__ __forceinline__ int4 axis_record(int d, int n, int S) {
    const int64_t num = (int64_t)(2 * d + 1) * n - S;
    int s = num < 0 ? -1 : (int)(num / (2 * S));
    int w1 = 0;
    if (s < 0) {
        s = 0;
    } else if (s >= n - 1) {
        s = n - 1;
    } else {
        const int frac = (int)(num - (int64_t)2 * S * s);
        w1 = (frac * TC_WONE + S) / (2 * S);
    }
    return make_int4(s, min(s + 1, n - 1), w1, (int)(((int64_t)d * n) / S));
}

template <typename T, bool VEC>
__global__ __launch_bounds__(TC_THREADS) void train_crop_kernel(const uint8_t* __restrict__ color, const T* __restrict__ raw,
                                                                const float* __restrict__ xyz, int32_t* __restrict__ boxes,
                                                                uint8_t* __restrict__ color_out, T* __restrict__ raw_out,
                                                                float* __restrict__ xyz_out, int H, int W, int Hp, int Wp, int S, int Sp) {
    __shared__ int4 s_col[TC_MAXS];
    const int b = blockIdx.y, tid = threadIdx.x;
    int x0 = boxes[b * CB_ROW], y0 = boxes[b * CB_ROW + 1], x1 = boxes[b * CB_ROW + 2], y1 = boxes[b * CB_ROW + 3];
    const bool ok = x0 >= 0 && x0 < x1 && x1 <= W - 1 && y0 >= 0 && y0 < y1 && y1 <= H - 1;
    if (!ok) {                                                                 // nothing of this row is used: zeros and a status bit
        if (blockIdx.x == 0 && tid == 0) atomicOr(&boxes[b * CB_ROW + 7], MSM_CROP_BAD_BOX);
        x0 = y0 = 0;
        x1 = y1 = 1;
    }
    const int nx = x1 - x0 + 1, ny = y1 - y0 + 1;                              // in [2, W] and [2, H] from here on
    for (int d = tid; d < S; d += TC_THREADS) s_col[d] = axis_record(d, nx, S);
    __syncthreads();
    const int rows = xyz_out != nullptr ? Sp : S, width = rows;                // the xyz planes carry the zero padding
    const int groups = (width + 3) >> 2;
    const int wave = tid >> 6, lane = tid & 63;
    const int64_t in_plane = (int64_t)Hp * Wp, out_plane = (int64_t)Sp * Sp;
    const uint8_t* img = color + (int64_t)b * H * W * 3;
    const T* lab = raw + (int64_t)b * H * W;
    const float* pts = xyz != nullptr ? xyz + (int64_t)b * 3 * in_plane : nullptr;
    const int row_end = min((int)(blockIdx.x + 1) * TC_BAND, rows);
    for (int dy = blockIdx.x * TC_BAND + wave; dy < row_end; dy += TC_THREADS / 64) {
        const bool row_in = ok && dy < S;
        const int4 ry = axis_record(row_in ? dy : 0, ny, S);                   // wave-uniform
        const uint8_t* c0 = img + ((int64_t)(y0 + ry.x) * W + x0) * 3;          // only dereferenced under row_in
        const uint8_t* c1 = img + ((int64_t)(y0 + ry.y) * W + x0) * 3;
        const T* l0 = lab + (int64_t)(y0 + ry.w) * W + x0;
        const int64_t p0 = (int64_t)(y0 + ry.w) * Wp + x0;
        const uint32_t wy1 = (uint32_t)ry.z, wy0 = TC_WONE - wy1;
        for (int g = lane; g < groups; g += 64) {
            const int dx0 = g * 4;
            uint32_t cpix[4][3];
            T lpix[4];
            float zpix[3][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int dx = dx0 + k;
                cpix[k][0] = cpix[k][1] = cpix[k][2] = 0u;
                lpix[k] = (T)0;
                zpix[0][k] = zpix[1][k] = zpix[2][k] = 0.f;
                if (row_in && dx < S) {
                    const int4 rx = s_col[dx];
                    const uint32_t wx1 = (uint32_t)rx.z, wx0 = TC_WONE - wx1;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const uint32_t a = c0[rx.x * 3 + ch], bb = c0[rx.y * 3 + ch], c = c1[rx.x * 3 + ch], d = c1[rx.y * 3 + ch];
                        cpix[k][ch] = ((a * wx0 + bb * wx1) * wy0 + (c * wx0 + d * wx1) * wy1 + (1u << (2 * TC_WBITS - 1))) >> (2 * TC_WBITS);
                    }
                    lpix[k] = l0[rx.w];
                    if (pts != nullptr) {
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) zpix[ch][k] = pts[ch * in_plane + p0 + rx.w];
                    }
                }
            }
            if (dy < S && dx0 < S) {
                const int64_t o = ((int64_t)b * S + dy) * S + dx0;
                if (VEC) {                                                     // S % 4 == 0: the four pixels lie inside
                    uint32_t by[12];
#pragma unroll
                    for (int k = 0; k < 4; ++k)
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) by[k * 3 + ch] = cpix[k][ch];
                    uint32_t* cw = reinterpret_cast<uint32_t*>(color_out + o * 3);
#pragma unroll
                    for (int j = 0; j < 3; ++j) cw[j] = by[4 * j] | (by[4 * j + 1] << 8) | (by[4 * j + 2] << 16) | (by[4 * j + 3] << 24);
                    if (sizeof(T) == 1) {
                        *reinterpret_cast<uint32_t*>(raw_out + o) = (uint32_t)lpix[0] | ((uint32_t)lpix[1] << 8) | ((uint32_t)lpix[2] << 16) |
                                                                    ((uint32_t)lpix[3] << 24);
                    } else {
                        *reinterpret_cast<int4*>(raw_out + o) = make_int4((int)lpix[0], (int)lpix[1], (int)lpix[2], (int)lpix[3]);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (dx0 + k < S) {
#pragma unroll
                            for (int ch = 0; ch < 3; ++ch) color_out[(o + k) * 3 + ch] = (uint8_t)cpix[k][ch];
                            raw_out[o + k] = lpix[k];
                        }
                    }
                }
            }
            if (xyz_out != nullptr) {                                          // dy < Sp and dx0 < Sp here
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    float* zo = xyz_out + ((int64_t)b * 3 + ch) * out_plane + (int64_t)dy * Sp + dx0;
                    if (VEC) {
                        *reinterpret_cast<float4*>(zo) = make_float4(zpix[ch][0], zpix[ch][1], zpix[ch][2], zpix[ch][3]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (dx0 + k < Sp) zo[k] = zpix[ch][k];
                    }
                }
            }
        }
    }
}

template <typename T>
void launch_crop(dim3 grid, hipStream_t s, bool vec, const uint8_t* color, const T* raw, const float* xyz, int32_t* boxes,
                 uint8_t* color_out, T* raw_out, float* xyz_out, int H, int W, int Hp, int Wp, int S, int Sp) {
    if (vec)
        hipLaunchKernelGGL((train_crop_kernel<T, true>), grid, dim3(TC_THREADS), 0, s, color, raw, xyz, boxes, color_out, raw_out, xyz_out,
                           H, W, Hp, Wp, S, Sp);
    else
        hipLaunchKernelGGL((train_crop_kernel<T, false>), grid, dim3(TC_THREADS), 0, s, color, raw, xyz, boxes, color_out, raw_out, xyz_out,
                           H, W, Hp, Wp, S, Sp);
}

bool crop_shape_ok(int B, int H, int W) {
    return B > 0 && B <= 65535 && H >= 2 && W >= 2 && (int64_t)H * W <= ((int64_t)1 << 24);
}

}  // namespace

extern "C" int msm_crop_boxes(const int32_t* tables, const int32_t* params, int32_t* boxes, int B, int H, int W, void* stream) {
    MSM_REQUIRE(tables && params && boxes, "msm_crop_boxes: null pointer");
    MSM_REQUIRE(crop_shape_ok(B, H, W), "msm_crop_boxes: bad shape B=%d H=%d W=%d (B <= 65535, H, W >= 2, H W <= 2^24)", B, H, W);
    MSM_REQUIRE((((uintptr_t)tables | (uintptr_t)params) & 3) == 0 && ((uintptr_t)boxes & 15) == 0,
                "msm_crop_boxes: misaligned pointer (boxes: 16 bytes)");
    hipLaunchKernelGGL(crop_boxes_kernel, dim3(msm::cdiv(B, CB_THREADS)), dim3(CB_THREADS), 0, (hipStream_t)stream, tables, params, boxes,
                       B, H, W);
    MSM_CHECK_LAUNCH("msm_crop_boxes");
    return MSM_OK;
}

extern "C" int msm_train_crop(const uint8_t* color, const void* raw, int raw_is_i32, const float* xyz, int32_t* boxes, uint8_t* color_out,
                              void* raw_out, float* xyz_out, int B, int H, int W, int Hp, int Wp, int S, int Sp, void* stream) {
    MSM_REQUIRE(color && raw && boxes && color_out && raw_out, "msm_train_crop: null pointer");
    MSM_REQUIRE((xyz == nullptr) == (xyz_out == nullptr), "msm_train_crop: xyz and xyz_out go together");
    MSM_REQUIRE(crop_shape_ok(B, H, W), "msm_train_crop: bad shape B=%d H=%d W=%d (B <= 65535, H, W >= 2, H W <= 2^24)", B, H, W);
    MSM_REQUIRE(S >= 1 && S <= Sp && S <= TC_MAXS && Sp <= 2 * TC_MAXS, "msm_train_crop: bad size S=%d Sp=%d (1 <= S <= Sp, S <= %d, Sp <= %d)",
                S, Sp, TC_MAXS, 2 * TC_MAXS);
    MSM_REQUIRE(xyz == nullptr || (Hp >= H && Wp >= W && (int64_t)Hp * Wp <= ((int64_t)1 << 26)),
                "msm_train_crop: the xyz frame %dx%d must hold the image %dx%d (and at most 2^26 pixels)", Hp, Wp, H, W);
    MSM_REQUIRE((((uintptr_t)boxes | (uintptr_t)xyz | (uintptr_t)xyz_out) & 3) == 0 &&
                    (!raw_is_i32 || (((uintptr_t)raw | (uintptr_t)raw_out) & 3) == 0),
                "msm_train_crop: misaligned pointer");
    const bool vec = S % 4 == 0 && (xyz_out == nullptr || Sp % 4 == 0) &&
                     (((uintptr_t)color_out | (uintptr_t)raw_out | (uintptr_t)xyz_out) & 15) == 0;
    const int rows = xyz_out != nullptr ? Sp : S;
    const dim3 grid((unsigned)msm::cdiv(rows, TC_BAND), (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    if (raw_is_i32)
        launch_crop(grid, s, vec, color, static_cast<const int32_t*>(raw), xyz, boxes, color_out, static_cast<int32_t*>(raw_out), xyz_out, H, W,
                    Hp, Wp, S, Sp);
    else
        launch_crop(grid, s, vec, color, static_cast<const uint8_t*>(raw), xyz, boxes, color_out, static_cast<uint8_t*>(raw_out), xyz_out, H, W,
                    Hp, Wp, S, Sp);
    MSM_CHECK_LAUNCH("msm_train_crop");
    return MSM_OK;
}
