// The random augmentations of the reference's training loader for a batch of frames (TableTopDataset.__getitem__
// lib/datasets/tabletop_dataset.py:161-181,364-367: chromatic_transform / add_noise lib/utils/blob.py:74-129, add_noise_to_depth /
// dropout_random_ellipses / add_noise_to_xyz lib/utils/augmentation.py:58-126).  Every random number is drawn by the caller and
// arrives in the per-image table (augment.pack_table) or in a noise field; the kernels are pure functions of their inputs, and
// the definitions D1-D5 (include/msm_hip.h, augment.py) are float32 / integer steps in a fixed order, one rounding per written
// operation.  The whole file is compiled without contraction (the pragma below): no multiply-add, no reciprocal; divisions
// are hipcc's correctly rounded ones.  The numpy host path of augment.py is the definition, and these kernels equal it bit
// for bit.
//
//   msm_augment_color   one launch; a workgroup takes a 16 x 64 pixel tile of one image.  The image's mode is a uniform branch
//                       read once from its table row.  Without blur a lane takes four pixels of a row: D1, then D2, 12 bytes
//                       in and out as three dwords where W % 4 == 0 and the pointers allow, bytes otherwise.  With blur the
//                       workgroup converts its tile plus the halo on the blurred axis with D1 once into LDS (reflect-101 is
//                       applied when the halo is filled), then every lane sums its taps from LDS in integers.
//   msm_augment_depth   three launches, no host round trip, no float atomics: (a1) the valid pixels per row, a wave per four rows
//                       over the whole chip (integer compares against a per-image threshold: see depth_threshold); (a2) one
//                       workgroup per image scans the row counts and resolves the <= 32 centre ranks (a wave per ellipse:
//                       binary search over the row prefix, then a ballot / popcount walk along the one row) into a record
//                       block per image; (b) every lane scales four pixels and tests them against the image's records,
//                       staged in LDS with each ellipse's bounding box first.  All counts are integers; nothing depends on
//                       arrival order.  (Counting inside (a2) -- one workgroup reading a whole image -- took 36 us at
//                       8 x 480 x 640 however its loads were issued: one CU's issue rate, not memory.)
//   msm_xyz_noise       one launch, in place: a workgroup sums the few source rows of its 16 x 64 tile along x once into LDS, a
//                       pixel then reads four of them per channel; indices and weights from a host-built table.
// Every index read from a device table is bounded before use; a row that cannot be carried out is skipped and recorded in the
// status words (the convention of msm_target_write).
#include <float.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int ROW = MSM_AUGMENT_TABLE_ROW;
constexpr int EMAX = MSM_AUGMENT_ELLIPSE_MAX;
constexpr int REC_HEAD = 8, REC_WORDS = 12;
constexpr int REC_ROW = REC_HEAD + EMAX * REC_WORDS;      // int32 words per image
static_assert(REC_ROW == MSM_AUGMENT_RECORD_ROW, "the record block of msm_hip.h");
enum { COL_FLAGS = 0, COL_BLUR_SIZE, COL_BLUR_HORIZONTAL, COL_D_H, COL_D_L, COL_D_S, COL_SIGMA, COL_MULTIPLIER, COL_COUNT, COL_ELLIPSES = 16 };
enum { F_CHROMATIC = 1, F_GAUSSIAN = 2, F_BLUR = 4, F_DEPTH = 8 };
enum { AUG_U16 = 1, AUG_F32 = 2 };

__device__ __forceinline__ float as_f(int32_t v) { return __int_as_float(v); }

// ---------------------------------------------------------------------------------------------------------------- D1
// The five divisions of a byte by 255 and the one of H' 6 by 180 are read from two tables the workgroup fills with those very
// divisions (lut255[v] = float(v) / 255, lut_h[v] = (float(v) * 6) / 180): the same values, two divisions per pixel left.
__device__ __forceinline__ void chroma_px(uint8_t& pb, uint8_t& pg, uint8_t& pr, float dh, float dl, float ds,
                                          const float* __restrict__ lut255, const float* __restrict__ lut_h) {
    const float bf = lut255[pb], gf = lut255[pg], rf = lut255[pr];
    const float vmax = fmaxf(fmaxf(bf, gf), rf), vmin = fminf(fminf(bf, gf), rf);
    const float sm = vmax + vmin, diff = vmax - vmin;
    const float l = sm * 0.5f;
    float h = 0.f, s = 0.f;
    if (diff > FLT_EPSILON) {
        s = l < 0.5f ? diff / sm : diff / ((2.f - vmax) - vmin);
        const float k = 60.f / diff;
        if (vmax == rf) h = (gf - bf) * k;
        else if (vmax == gf) h = (bf - rf) * k + 120.f;
        else h = (rf - gf) * k + 240.f;
        if (h < 0.f) h = h + 360.f;
        h = h * 0.5f;
    }
    const float H8 = rintf(h), L8 = rintf(l * 255.f), S8 = rintf(s * 255.f);
    // shift: numpy's float32 mod(x, 180) for x in [-360, 360] -- the first step is exact, the second rounds (and can give 180)
    float x = H8 + dh;
    if (x >= 360.f) x = x - 360.f;
    else if (x >= 180.f) x = x - 180.f;
    else if (x <= -180.f) x = x + 180.f;
    if (x < 0.f) x = x + 180.f;
    const float Hn = truncf(x);
    const float Ln = truncf(fminf(fmaxf(L8 + dl, 0.f), 255.f));
    const float Sn = truncf(fminf(fmaxf(S8 + ds, 0.f), 255.f));
    // back
    const float l2 = lut255[(int)Ln], s2 = lut255[(int)Sn];           // Ln, Sn in [0, 255] by the clip
    float ob = l2, og = l2, orr = l2;
    if (s2 != 0.f) {
        const float p2 = l2 <= 0.5f ? l2 * (1.f + s2) : (l2 + s2) - l2 * s2;
        const float p1 = 2.f * l2 - p2;
        const float d = p2 - p1;
        float hh = lut_h[min(max((int)Hn, 0), 180)];
        if (hh >= 6.f) hh = hh - 6.f;
        const float sec = fminf(fmaxf(floorf(hh), 0.f), 5.f);
        const float f = hh - sec;
        const float t2 = p1 + d * (1.f - f), t3 = p1 + d * f;
        switch ((int)sec) {
            case 0: ob = p1; og = t3; orr = p2; break;
            case 1: ob = p1; og = p2; orr = t2; break;
            case 2: ob = t3; og = p2; orr = p1; break;
            case 3: ob = p2; og = t2; orr = p1; break;
            case 4: ob = p2; og = p1; orr = t3; break;
            default: ob = t2; og = p1; orr = p2; break;
        }
    }
    pb = (uint8_t)fminf(fmaxf(rintf(ob * 255.f), 0.f), 255.f);
    pg = (uint8_t)fminf(fmaxf(rintf(og * 255.f), 0.f), 255.f);
    pr = (uint8_t)fminf(fmaxf(rintf(orr * 255.f), 0.f), 255.f);
}

constexpr int CT_W = 64, CT_H = 16, C_THREADS = 256, C_HALO = 7;
constexpr int C_LDS = (CT_H + 2 * C_HALO) * CT_W * 3;    // the vertical halo is the larger region: 30 x 64 pixels (16 x 78 horizontal)

template <bool VEC>
__global__ __launch_bounds__(C_THREADS) void augment_color_kernel(const uint8_t* __restrict__ color, const int32_t* __restrict__ table,
                                                                  const float* __restrict__ noise, uint8_t* __restrict__ out,
                                                                  int32_t* __restrict__ status, int H, int W) {
    __shared__ uint8_t tile[C_LDS];
    __shared__ float lut255[256];
    __shared__ float lut_h[181];
    const int b = blockIdx.z;
    const int32_t* row = table + (int64_t)b * ROW;
    int flags = row[COL_FLAGS];
    const int size = row[COL_BLUR_SIZE], horiz = row[COL_BLUR_HORIZONTAL];
    const float dh = as_f(row[COL_D_H]), dl = as_f(row[COL_D_L]), ds = as_f(row[COL_D_S]), sigma = as_f(row[COL_SIGMA]);
    bool ok = (flags & ~15) == 0 && !((flags & F_GAUSSIAN) && (flags & F_BLUR));
    if (flags & F_CHROMATIC) ok = ok && fabsf(dh) <= 180.f && fabsf(dl) <= 512.f && fabsf(ds) <= 512.f;
    if (flags & F_GAUSSIAN) ok = ok && fabsf(sigma) <= 65536.f && noise != nullptr;
    if (flags & F_BLUR) {
        const bool known = size == 3 || size == 5 || size == 7 || size == 9 || size == 11 || size == 15;
        ok = ok && known && (horiz == 0 || horiz == 1) && (horiz ? W : H) > (size >> 1);
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) status[b * 4 + 0] = ok ? 0 : MSM_AUGMENT_BAD_ROW;
    if (!ok) flags = 0;                                   // a row that cannot be carried out copies its image
    if (flags & F_CHROMATIC) {                            // (uniform)
        lut255[threadIdx.x] = (float)threadIdx.x / 255.f;
        if (threadIdx.x <= 180) lut_h[threadIdx.x] = ((float)threadIdx.x * 6.f) / 180.f;
        __syncthreads();
    }
    const int tx0 = blockIdx.x * CT_W, ty0 = blockIdx.y * CT_H;
    const int ly = threadIdx.x >> 4, lx = (threadIdx.x & 15) * 4;
    const int y = ty0 + ly, x0 = tx0 + lx;
    const int64_t img = (int64_t)b * H * W;
    uint8_t px[4][3];
    bool in[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) in[i] = y < H && x0 + i < W;
    if (flags & F_BLUR) {
        const int half = size >> 1, hx = horiz ? half : 0, hy = horiz ? 0 : half;
        const int RW = CT_W + 2 * hx, RH = CT_H + 2 * hy;
        for (int i = threadIdx.x; i < RW * RH; i += C_THREADS) {
            const int ry = i / RW, rx = i - ry * RW;
            int gy = ty0 - hy + ry, gx = tx0 - hx + rx;
            if (gy >= H + hy || gx >= W + hx) continue;   // (gy >= -hy and gx >= -hx by construction)
            gy = gy < 0 ? -gy : gy;
            gy = gy >= H ? 2 * H - 2 - gy : gy;           // reflect-101; in range because the extent exceeds the halo
            gx = gx < 0 ? -gx : gx;
            gx = gx >= W ? 2 * W - 2 - gx : gx;
            const uint8_t* p = color + (img + (int64_t)gy * W + gx) * 3;
            uint8_t c0 = p[0], c1 = p[1], c2 = p[2];
            if (flags & F_CHROMATIC) chroma_px(c0, c1, c2, dh, dl, ds, lut255, lut_h);
            tile[i * 3 + 0] = c0;
            tile[i * 3 + 1] = c1;
            tile[i * 3 + 2] = c2;
        }
        __syncthreads();
        const int step = (horiz ? 1 : RW) * 3;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!in[i]) continue;
            const uint8_t* t0 = tile + (ly * RW + lx + i) * 3;   // tap 0 = position - half: the region starts there
            int s0 = 0, s1 = 0, s2 = 0;
            for (int k = 0; k < size; ++k) {
                s0 += t0[k * step + 0];
                s1 += t0[k * step + 1];
                s2 += t0[k * step + 2];
            }
            px[i][0] = (uint8_t)((2 * s0 + size) / (2 * size));
            px[i][1] = (uint8_t)((2 * s1 + size) / (2 * size));
            px[i][2] = (uint8_t)((2 * s2 + size) / (2 * size));
        }
    } else {
        if (!in[0]) return;
        const int64_t pix = img + (int64_t)y * W + x0;
        float nz[4] = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {                                        // W % 4 == 0: the quad is inside as a whole
            const uint32_t* cp = reinterpret_cast<const uint32_t*>(color + pix * 3);
            const uint32_t w0 = cp[0], w1 = cp[1], w2 = cp[2];
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                const uint32_t w = k < 4 ? w0 : (k < 8 ? w1 : w2);
                px[k / 3][k % 3] = (uint8_t)(w >> (8 * (k & 3)));
            }
            if (flags & F_GAUSSIAN) {
                const float4 n4 = *reinterpret_cast<const float4*>(noise + pix);
                nz[0] = n4.x; nz[1] = n4.y; nz[2] = n4.z; nz[3] = n4.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                px[i][0] = px[i][1] = px[i][2] = 0;
                if (in[i]) {
                    const uint8_t* cp = color + (pix + i) * 3;
                    px[i][0] = cp[0]; px[i][1] = cp[1]; px[i][2] = cp[2];
                    if (flags & F_GAUSSIAN) nz[i] = noise[pix + i];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!in[i]) continue;
            if (flags & F_CHROMATIC) chroma_px(px[i][0], px[i][1], px[i][2], dh, dl, ds, lut255, lut_h);
            if (flags & F_GAUSSIAN) {
                const float t = sigma * nz[i];
#pragma unroll
                for (int c = 0; c < 3; ++c) px[i][c] = (uint8_t)truncf(fminf(fmaxf((float)px[i][c] + t, 0.f), 255.f));
            }
        }
    }
    if (!in[0]) return;
    const int64_t pix = img + (int64_t)y * W + x0;
    if (VEC) {
        uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k >> 2] |= (uint32_t)px[k / 3][k % 3] << (8 * (k & 3));
        uint32_t* op = reinterpret_cast<uint32_t*>(out + pix * 3);
        op[0] = w[0]; op[1] = w[1]; op[2] = w[2];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (in[i]) {
                uint8_t* op = out + (pix + i) * 3;
                op[0] = px[i][0]; op[1] = px[i][1]; op[2] = px[i][2];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- D4
template <int DK>
__device__ __forceinline__ float depth_z(const void* __restrict__ depth, int64_t i, float div, float m) {
    float z;
    if (DK == AUG_U16) {
        z = (float)static_cast<const uint16_t*>(depth)[i] / div;
    } else {
        z = static_cast<const float*>(depth)[i];
        z = z != z ? 0.f : z;                              // NaN -> 0, as msm_ingest_frames
    }
    return z * m;
}

// "z > 0" of pixel i without its division.  For uint16 depth the predicate P(d) = ((float(d) / div) * m > 0) is monotone in d when
// m > 0 (both roundings are monotone) and false for every d when m <= 0, so it is d >= thr with thr the smallest d that satisfies
// it (65536: none), found once per image by bisection on the very expression.  One workgroup reads a whole image in launch (a):
// eight divisions per 16-byte load kept its one CU busy for 40 us at 480 x 640.
__device__ __forceinline__ uint32_t depth_threshold(float div, float m) {
    uint32_t lo = 1, hi = 65536;
    if (!(m > 0.f)) return hi;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;                 // < 65536
        if (((float)mid / div) * m > 0.f) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

template <int DK>
__device__ __forceinline__ bool depth_valid(const void* __restrict__ depth, int64_t i, uint32_t thr, float m) {
    if (DK == AUG_U16) return static_cast<const uint16_t*>(depth)[i] >= thr;
    const float z = static_cast<const float*>(depth)[i];
    return (z != z ? 0.f : z) * m > 0.f;
}

// What a table row asks of its depth map: the ellipse count (0: none, or the row is skipped), the multiplier and the status bits.
struct DepthMode {
    int count;
    float m;
    int st;
};
__device__ __forceinline__ DepthMode depth_mode(const int32_t* __restrict__ row) {
    DepthMode md = {row[COL_COUNT], as_f(row[COL_MULTIPLIER]), 0};
    if (!(row[COL_FLAGS] & F_DEPTH)) {
        md.count = 0;
        md.m = 1.f;
    } else {
        if (!(fabsf(md.m) <= FLT_MAX)) md.st |= MSM_AUGMENT_BAD_ROW;
        if (md.count < 0 || md.count > EMAX) md.st |= MSM_AUGMENT_BAD_COUNT;
        if (md.st) {                                       // skipped: the map is only converted
            md.count = 0;
            md.m = 1.f;
        }
    }
    return md;
}

constexpr int DR_THREADS = 256, DR_ROWS = 4;               // rows per wave: a workgroup of four waves counts 16 rows

// (a1) valid pixels per row, a wave per DR_ROWS consecutive rows (one contiguous stretch of memory), 16-byte loads where
// W % 8 == 0.  Images without ellipses are left alone: nobody reads their counts.
template <int DK, bool VEC>
__global__ __launch_bounds__(DR_THREADS) void augment_depth_rows_kernel(const void* __restrict__ depth, float div, const int32_t* __restrict__ table,
                                                                        uint32_t* __restrict__ rowcnt, int H, int W) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const DepthMode md = depth_mode(table + (int64_t)b * ROW);
    if (md.count <= 0) return;                             // (uniform)
    const uint32_t thr = DK == AUG_U16 ? depth_threshold(div, md.m) : 0u;
    const float m = md.m;
    const int y0 = (blockIdx.x * (DR_THREADS / 64) + wave) * DR_ROWS, nr = min(DR_ROWS, H - y0);
    if (nr <= 0) return;
    const int64_t base = ((int64_t)b * H + y0) * W;
    uint32_t c[DR_ROWS];
#pragma unroll
    for (int k = 0; k < DR_ROWS; ++k) c[k] = 0;
    if (VEC) {                                             // W % 8 == 0: a chunk of eight pixels lies in one row
        const int per_row = W >> 3, chunks = nr * per_row;
#pragma unroll 4
        for (int j = lane; j < chunks; j += 64) {
            const uint4* src = reinterpret_cast<const uint4*>(static_cast<const char*>(depth) + (base + (int64_t)j * 8) * (DK == AUG_U16 ? 2 : 4));
            uint32_t cnt = 0;
            if (DK == AUG_U16) {
                const uint4 d = src[0];
                const uint32_t wd[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) cnt += ((wd[k] & 0xffffu) >= thr ? 1u : 0u) + ((wd[k] >> 16) >= thr ? 1u : 0u);
            } else {
                const uint4 d0 = src[0], d1 = src[1];
                const uint32_t wd[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float v = __uint_as_float(wd[k]);
                    cnt += (v != v ? 0.f : v) * m > 0.f ? 1u : 0u;
                }
            }
            const int r = j / per_row;
#pragma unroll
            for (int k = 0; k < DR_ROWS; ++k) c[k] += r == k ? cnt : 0u;
        }
    } else {
#pragma unroll
        for (int k = 0; k < DR_ROWS; ++k) {
            if (k >= nr) break;
            for (int x = lane; x < W; x += 64) c[k] += depth_valid<DK>(depth, base + (int64_t)k * W + x, thr, m) ? 1u : 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < DR_ROWS; ++k) {
        uint32_t v = c[k];
        for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0 && k < nr) rowcnt[(int64_t)b * H + y0 + k] = v;
    }
}

constexpr int DA_THREADS = 1024, DA_WAVES = DA_THREADS / 64, DA_UNROLL = 8, D_MAX_H = MSM_AUGMENT_MAX_H;

// (a2) one workgroup per image: the exclusive prefix of the row counts, the centres of the image's ellipses -> records.
template <int DK>
__global__ __launch_bounds__(DA_THREADS) void augment_depth_centres_kernel(const void* __restrict__ depth, float div,
                                                                           const int32_t* __restrict__ table, const uint32_t* __restrict__ rowcnt,
                                                                           int32_t* __restrict__ records, int32_t* __restrict__ status, int H, int W) {
    __shared__ uint32_t rowpre[D_MAX_H];
    __shared__ uint32_t part[DA_WAVES];
    __shared__ uint32_t total_s;
    __shared__ int st_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* row = table + (int64_t)b * ROW;
    int32_t* rec = records + (int64_t)b * REC_ROW;
    const DepthMode md = depth_mode(row);
    const int count = md.count;
    const float m = md.m;
    if (tid == 0) st_s = md.st;
    const int64_t img = (int64_t)b * H * W;
    uint32_t n = 0;
    const uint32_t thr = DK == AUG_U16 && count > 0 ? depth_threshold(div, m) : 0u;
    if (count > 0) {                                       // (uniform) without ellipses nobody needs the counts
        for (int y = tid; y < H; y += DA_THREADS) rowpre[y] = rowcnt[(int64_t)b * H + y];
        __syncthreads();
        // exclusive scan of the row counts: a run of rows per thread, a wave scan, a scan of the sixteen wave totals
        const int per = (H + DA_THREADS - 1) / DA_THREADS;
        const int r0 = min(H, tid * per), r1 = min(H, r0 + per);
        uint32_t mysum = 0;
        for (int r = r0; r < r1; ++r) mysum += rowpre[r];
        uint32_t inc = mysum;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) part[wave] = inc;
        __syncthreads();
        if (wave == 0) {
            const uint32_t p = lane < DA_WAVES ? part[lane] : 0u;
            uint32_t pi = p;
            for (int o = 1; o < DA_WAVES; o <<= 1) {
                const uint32_t t = __shfl_up(pi, o, 64);
                if (lane >= o) pi += t;
            }
            if (lane < DA_WAVES) part[lane] = pi - p;
            if (lane == DA_WAVES - 1) total_s = pi;
        }
        __syncthreads();
        uint32_t run = part[wave] + inc - mysum;
        for (int r = r0; r < r1; ++r) {
            const uint32_t c = rowpre[r];
            rowpre[r] = run;
            run += c;
        }
        __syncthreads();
        n = total_s;
    } else {
        __syncthreads();                                   // st_s
    }
    for (int i = wave; i < count; i += DA_WAVES) {         // count <= EMAX: the table reads stay inside the row
        const int32_t* e = row + COL_ELLIPSES + MSM_AUGMENT_ELLIPSE_WORDS * i;
        const float rx = as_f(e[0]), ry = as_f(e[1]), c = as_f(e[2]), s = as_f(e[3]);
        const uint32_t key = (uint32_t)e[4];
        const bool ok = rx >= 0.f && rx <= 65536.f && ry >= 0.f && ry <= 65536.f && fabsf((c * c + s * s) - 1.f) <= 1e-3f;
        int cx = 0, cy = 0;
        bool found = false;
        if (!ok) {
            if (lane == 0) atomicOr(&st_s, MSM_AUGMENT_BAD_ELLIPSE);
        } else if (n > 0) {
            const uint32_t rank = (uint32_t)(((uint64_t)key * (uint64_t)n) >> 32);      // < n
            int lo = 0, hi = H - 1;                        // the last row whose prefix is <= rank holds that pixel
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (rowpre[mid] <= rank) lo = mid;
                else hi = mid - 1;
            }
            cy = lo;
            uint32_t rem = rank - rowpre[cy];
            bool done = false;
            for (int xb = 0; xb < W && !done; xb += 64 * DA_UNROLL) {      // DA_UNROLL chunks of 64 pixels loaded together
                bool v[DA_UNROLL];
#pragma unroll
                for (int u = 0; u < DA_UNROLL; ++u) {
                    const int x = xb + u * 64 + lane;
                    v[u] = depth_valid<DK>(depth, img + (int64_t)cy * W + min(x, W - 1), thr, m) && x < W;
                }
#pragma unroll
                for (int u = 0; u < DA_UNROLL; ++u) {
                    if (done) break;
                    const uint64_t mask = __ballot(v[u]);
                    const uint32_t cnt = (uint32_t)__popcll(mask);
                    if (rem < cnt) {
                        const bool mine = v[u] && (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)) == rem;
                        const uint64_t who = __ballot(mine);
                        found = who != 0;
                        cx = xb + u * 64 + (found ? __ffsll((long long)who) - 1 : 0);
                        done = true;
                    } else {
                        rem -= cnt;
                    }
                }
            }
        }
        if (lane == 0) {
            int32_t* o = rec + REC_HEAD + REC_WORDS * i;
            const float a = fmaxf(rx, 0.5f), bb = fmaxf(ry, 0.5f);
            // |dx|, |dy| <= max(a, b) / sqrt(cos^2 + sin^2) inside the ellipse: the box is generous, never decisive
            const int R = found ? (int)ceilf(fmaxf(a, bb) * 1.01f + 1.f) : -1;
            o[0] = cx; o[1] = cy;
            o[2] = cx - R; o[3] = cx + R; o[4] = cy - R; o[5] = cy + R;           // not found: an empty box
            o[6] = __float_as_int(a * a); o[7] = __float_as_int(bb * bb);
            o[8] = __float_as_int(c); o[9] = __float_as_int(s);
            o[10] = 0; o[11] = 0;
        }
    }
    __syncthreads();
    if (tid == 0) {
        rec[0] = count;
        rec[1] = (int32_t)n;
        rec[2] = __float_as_int(m);
        for (int k = 3; k < REC_HEAD; ++k) rec[k] = 0;
        status[b * 4 + 1] = st_s;
    }
}

constexpr int DB_THREADS = 256;

// (b) four pixels per lane: scale, test against the image's records, store.
template <int DK, bool VEC>
__global__ __launch_bounds__(DB_THREADS) void augment_depth_apply_kernel(const void* __restrict__ depth, float div,
                                                                         const int32_t* __restrict__ records, float* __restrict__ out,
                                                                         int32_t* __restrict__ status, int H, int W, int Q, int quads) {
    __shared__ int32_t rec[REC_ROW];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int32_t* g = records + (int64_t)b * REC_ROW;
    const int count = min(max(g[0], 0), EMAX);             // bounded: the records are a device table like any other
    for (int i = tid; i < REC_HEAD + REC_WORDS * count; i += DB_THREADS) rec[i] = g[i];
    __syncthreads();
    if (tid < count) {
        int32_t* e = rec + REC_HEAD + REC_WORDS * tid;
        if (e[2] <= e[3] && e[4] <= e[5] && (e[0] < 0 || e[0] >= W || e[1] < 0 || e[1] >= H)) {
            e[2] = 1; e[3] = 0;                            // a centre outside the image: skipped and reported
            if (blockIdx.x == 0) atomicOr(&status[b * 4 + 1], MSM_AUGMENT_BAD_CENTRE);
        }
    }
    __syncthreads();
    const float m = as_f(rec[2]);
    const int64_t img = (int64_t)b * H * W;
    for (int q = blockIdx.x * DB_THREADS + tid; q < quads; q += gridDim.x * DB_THREADS) {
        const int y = q / Q, x0 = (q - y * Q) * 4;
        const int64_t pix = img + (int64_t)y * W + x0;
        float z[4];
        bool in[4];
        if (VEC) {
            if (DK == AUG_U16) {
                const uint2 d = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(depth) + pix);
                z[0] = (float)(d.x & 0xffffu); z[1] = (float)(d.x >> 16); z[2] = (float)(d.y & 0xffffu); z[3] = (float)(d.y >> 16);
#pragma unroll
                for (int i = 0; i < 4; ++i) z[i] = (z[i] / div) * m;
            } else {
                const float4 d = *reinterpret_cast<const float4*>(static_cast<const float*>(depth) + pix);
                z[0] = d.x; z[1] = d.y; z[2] = d.z; z[3] = d.w;
#pragma unroll
                for (int i = 0; i < 4; ++i) z[i] = (z[i] != z[i] ? 0.f : z[i]) * m;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) in[i] = true;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                in[i] = x0 + i < W;
                z[i] = in[i] ? depth_z<DK>(depth, pix + i, div, m) : 0.f;
            }
        }
        for (int k = 0; k < count; ++k) {
            const int32_t* e = rec + REC_HEAD + REC_WORDS * k;
            if (y < e[4] || y > e[5] || x0 + 3 < e[2] || x0 > e[3]) continue;
            const float a2 = as_f(e[6]), b2 = as_f(e[7]), c = as_f(e[8]), s = as_f(e[9]);
            const float dy = (float)(y - e[1]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float dx = (float)(x0 + i - e[0]);
                const float u = dx * c + dy * s, v = dy * c - dx * s;
                if ((u * u) / a2 + (v * v) / b2 <= 1.f) z[i] = 0.f;
            }
        }
        if (VEC) {
            *reinterpret_cast<float4*>(out + pix) = make_float4(z[0], z[1], z[2], z[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (in[i]) out[pix + i] = z[i];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- D5
constexpr int XT_W = 64, XT_H = 16, XT_ROWS = 12;

// One output pixel straight from the field: the four rows' sums along x, then the sum along y.
__device__ __forceinline__ void xyz_pixel_direct(float* __restrict__ p, int64_t plane, const float* __restrict__ gp, const int32_t* __restrict__ ty,
                                                 const int32_t* __restrict__ tx, float scale, int b, int h, int w) {
    int iy[4], ix[4];
    float wy[4], wx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        iy[j] = min(max(ty[j], 0), h - 1);                 // bounded whatever the table says
        ix[j] = min(max(tx[j], 0), w - 1);
        wy[j] = as_f(ty[4 + j]);
        wx[j] = as_f(tx[4 + j]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* g = gp + ((int64_t)b * 3 + c) * h * w;
        float rj[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* gr = g + (int64_t)iy[j] * w;
            rj[j] = ((wx[0] * gr[ix[0]] + wx[1] * gr[ix[1]]) + wx[2] * gr[ix[2]]) + wx[3] * gr[ix[3]];
        }
        const float up = ((wy[0] * rj[0] + wy[1] * rj[1]) + wy[2] * rj[2]) + wy[3] * rj[3];
        p[c * plane] = p[c * plane] + scale * up;
    }
}

// A workgroup takes a 16 x 64 tile of one image.  The sum along x of a source row depends on (source row, x) only, and a tile
// touches few source rows (7 for a 4x upsampling): they are computed once into LDS -- the same expression on the same operands as
// the direct form -- and a pixel then costs four LDS reads per channel instead of sixteen gathers.  A tile that spans more than
// XT_ROWS source rows (a field finer than the image) takes the direct form.
__global__ __launch_bounds__(256) void xyz_noise_kernel(float* __restrict__ xyz, const float* __restrict__ gp, const int32_t* __restrict__ taps,
                                                        float scale, int H, int W, int Hp, int Wp, int h, int w) {
    __shared__ float rows[3][XT_ROWS][XT_W];
    const int b = blockIdx.z, tx0 = blockIdx.x * XT_W, ty0 = blockIdx.y * XT_H;
    const int tid = threadIdx.x, xx = tid & 63, x = tx0 + xx;
    const int64_t plane = (int64_t)Hp * Wp;
    const int ylast = min(ty0 + XT_H, H) - 1;
    const int r_lo = min(max(taps[(int64_t)ty0 * 8], 0), h - 1), r_hi = min(max(taps[(int64_t)ylast * 8 + 3], 0), h - 1);
    const int nrows = r_hi - r_lo + 1;
    const int32_t* tx = taps + (int64_t)(H + min(x, W - 1)) * 8;
    if (nrows < 1 || nrows > XT_ROWS) {                    // (uniform)
        for (int ly = tid >> 6; ly < XT_H; ly += 4) {
            const int y = ty0 + ly;
            if (y >= H || x >= W) continue;
            float* p = xyz + ((int64_t)b * 3 * Hp + y) * Wp + x;
            if (p[2 * plane] > 0.f) xyz_pixel_direct(p, plane, gp, taps + (int64_t)y * 8, tx, scale, b, h, w);
        }
        return;
    }
    int ix[4];
    float wx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ix[j] = min(max(tx[j], 0), w - 1);
        wx[j] = as_f(tx[4 + j]);
    }
    for (int k = tid >> 6; k < 3 * nrows; k += 4) {        // (channel, source row) pairs; this lane's column throughout
        const int c = k / nrows, rr = k - c * nrows;
        const float* gr = gp + (((int64_t)b * 3 + c) * h + r_lo + rr) * w;
        rows[c][rr][xx] = ((wx[0] * gr[ix[0]] + wx[1] * gr[ix[1]]) + wx[2] * gr[ix[2]]) + wx[3] * gr[ix[3]];
    }
    __syncthreads();
    for (int ly = tid >> 6; ly < XT_H; ly += 4) {
        const int y = ty0 + ly;
        if (y >= H || x >= W) continue;
        float* p = xyz + ((int64_t)b * 3 * Hp + y) * Wp + x;
        if (!(p[2 * plane] > 0.f)) continue;
        const int32_t* ty = taps + (int64_t)y * 8;
        int ry[4];
        float wy[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ry[j] = min(max(min(max(ty[j], 0), h - 1) - r_lo, 0), nrows - 1);     // inside the staged rows whatever the table says
            wy[j] = as_f(ty[4 + j]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float up = ((wy[0] * rows[c][ry[0]][xx] + wy[1] * rows[c][ry[1]][xx]) + wy[2] * rows[c][ry[2]][xx]) + wy[3] * rows[c][ry[3]][xx];
            p[c * plane] = p[c * plane] + scale * up;
        }
    }
}

bool depth_shape_ok(int B, int H, int W) {
    return B > 0 && B <= 65535 && H > 0 && H <= D_MAX_H && W > 0 && W <= 65536 && (int64_t)B * H * W < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int msm_augment_table_row(void) { return ROW; }

extern "C" int msm_augment_color(const uint8_t* color, const int32_t* table, const float* noise, uint8_t* out, int32_t* status, int B,
                                 int H, int W, void* stream) {
    MSM_REQUIRE(color && table && out && status, "msm_augment_color: null pointer (color, table, out and status are required)");
    MSM_REQUIRE(color != out, "msm_augment_color: the blur reads its neighbours, out cannot be color");
    MSM_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)B * H * W < ((int64_t)1 << 31) && (H + CT_H - 1) / CT_H <= 65535,
                "msm_augment_color: bad shape B=%d H=%d W=%d", B, H, W);
    MSM_REQUIRE((((uintptr_t)table | (uintptr_t)noise | (uintptr_t)status) & 3) == 0, "msm_augment_color: misaligned pointer");
    const bool vec = W % 4 == 0 && (((uintptr_t)color | (uintptr_t)out) & 3) == 0 && ((uintptr_t)noise & 15) == 0;
    const dim3 grid(msm::cdiv(W, CT_W), msm::cdiv(H, CT_H), B);
    hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((augment_color_kernel<true>), grid, dim3(C_THREADS), 0, s, color, table, noise, out, status, H, W);
    else hipLaunchKernelGGL((augment_color_kernel<false>), grid, dim3(C_THREADS), 0, s, color, table, noise, out, status, H, W);
    MSM_CHECK_LAUNCH("msm_augment_color");
    return MSM_OK;
}

extern "C" int64_t msm_augment_depth_workspace(int B, int H, int W) {
    if (!depth_shape_ok(B, H, W)) {
        msm::set_error("msm_augment_depth_workspace: bad shape B=%d H=%d W=%d (H <= %d, W <= 65536, B <= 65535)", B, H, W, D_MAX_H);
        return MSM_E_INVALID;
    }
    return (int64_t)B * (REC_ROW + H) * 4;                  // the record blocks, then the row counts
}

template <int DK>
static int launch_depth(const void* depth, float div, const int32_t* table, float* out, int32_t* status, int32_t* records, int stages,
                        int B, int H, int W, hipStream_t s) {
    const int esz = DK == AUG_U16 ? 2 : 4;
    if (stages & 1) {
        uint32_t* rowcnt = reinterpret_cast<uint32_t*>(records + (int64_t)B * REC_ROW);
        const bool vec = W % 8 == 0 && ((uintptr_t)depth & 15) == 0;
        const dim3 grid(msm::cdiv(H, DR_ROWS * (DR_THREADS / 64)), B);
        if (vec) hipLaunchKernelGGL((augment_depth_rows_kernel<DK, true>), grid, dim3(DR_THREADS), 0, s, depth, div, table, rowcnt, H, W);
        else hipLaunchKernelGGL((augment_depth_rows_kernel<DK, false>), grid, dim3(DR_THREADS), 0, s, depth, div, table, rowcnt, H, W);
        MSM_CHECK_LAUNCH("msm_augment_depth (row counts)");
        hipLaunchKernelGGL((augment_depth_centres_kernel<DK>), dim3(B), dim3(DA_THREADS), 0, s, depth, div, table, rowcnt, records, status, H, W);
        MSM_CHECK_LAUNCH("msm_augment_depth (centres)");
    }
    if (stages & 2) {
        const int Q = msm::cdiv(W, 4), quads = H * Q;
        const bool vec = W % 4 == 0 && ((uintptr_t)depth & (4 * esz - 1)) == 0 && ((uintptr_t)out & 15) == 0;
        const dim3 grid(min(msm::cdiv(quads, DB_THREADS), 1024), B);
        if (vec) hipLaunchKernelGGL((augment_depth_apply_kernel<DK, true>), grid, dim3(DB_THREADS), 0, s, depth, div, records, out, status, H, W, Q, quads);
        else hipLaunchKernelGGL((augment_depth_apply_kernel<DK, false>), grid, dim3(DB_THREADS), 0, s, depth, div, records, out, status, H, W, Q, quads);
        MSM_CHECK_LAUNCH("msm_augment_depth (apply)");
    }
    return MSM_OK;
}

extern "C" int msm_augment_depth(const void* depth, int depth_is_u16, float depth_div, const int32_t* table, float* out,
                                 int32_t* status, void* workspace, int64_t workspace_bytes, int stages, int B, int H, int W,
                                 void* stream) {
    MSM_REQUIRE(depth && out && status && workspace, "msm_augment_depth: null pointer (depth, out, status and workspace are required)");
    MSM_REQUIRE(stages >= 1 && stages <= 3, "msm_augment_depth: stages must be 1 (centres), 2 (apply) or 3, got %d", stages);
    MSM_REQUIRE(table || !(stages & 1), "msm_augment_depth: the centres need the table");
    MSM_REQUIRE(depth_shape_ok(B, H, W), "msm_augment_depth: bad shape B=%d H=%d W=%d (H <= %d, W <= 65536, B <= 65535)", B, H, W, D_MAX_H);
    MSM_REQUIRE(depth_div > 0.f, "msm_augment_depth: depth_div must be positive");
    MSM_REQUIRE((((uintptr_t)table | (uintptr_t)out | (uintptr_t)status | (uintptr_t)workspace) & 3) == 0 &&
                    ((uintptr_t)depth & (depth_is_u16 ? 1 : 3)) == 0,
                "msm_augment_depth: misaligned pointer");
    if (workspace_bytes < (int64_t)B * (REC_ROW + H) * 4) {
        msm::set_error("msm_augment_depth: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)B * (REC_ROW + H) * 4);
        return MSM_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    int32_t* records = static_cast<int32_t*>(workspace);
    return depth_is_u16 ? launch_depth<AUG_U16>(depth, depth_div, table, out, status, records, stages, B, H, W, s)
                        : launch_depth<AUG_F32>(depth, depth_div, table, out, status, records, stages, B, H, W, s);
}

extern "C" int msm_xyz_noise(float* xyz, const float* gp, const int32_t* taps, float scale, int B, int H, int W, int Hp, int Wp, int h,
                             int w, void* stream) {
    MSM_REQUIRE(xyz && gp && taps, "msm_xyz_noise: null pointer");
    MSM_REQUIRE(B > 0 && H > 0 && W > 0 && Hp >= H && Wp >= W && h > 0 && w > 0 && (int64_t)B * Hp * Wp < ((int64_t)1 << 30) &&
                    (int64_t)B * 3 * h * w < ((int64_t)1 << 31) && (int64_t)H + W < ((int64_t)1 << 27),
                "msm_xyz_noise: bad shape B=%d H=%d W=%d frame %dx%d field %dx%d", B, H, W, Hp, Wp, h, w);
    MSM_REQUIRE((((uintptr_t)xyz | (uintptr_t)gp | (uintptr_t)taps) & 3) == 0, "msm_xyz_noise: misaligned pointer");
    MSM_REQUIRE(B <= 65535 && msm::cdiv(H, XT_H) <= 65535, "msm_xyz_noise: B=%d H=%d are too many for one launch", B, H);
    const dim3 grid(msm::cdiv(W, XT_W), msm::cdiv(H, XT_H), B);
    hipLaunchKernelGGL(xyz_noise_kernel, grid, dim3(256), 0, (hipStream_t)stream, xyz, gp, taps, scale, H, W, Hp, Wp, h, w);
    MSM_CHECK_LAUNCH("msm_xyz_noise");
    return MSM_OK;
}
