// Integer counts of the reference's segmentation metrics (lib/utils/evaluation.py:109-258 multilabel_metrics) for a batch
// of (prediction, ground truth) label-image pairs.
//
// The reference walks the image once per (gt label, predicted label) pair: masks, a joint count, two seg2bmap boundary maps
// (:46-57) and two disk dilations (boundary_overlap, :71-104).  Every number it derives is a ratio of exact integer counts,
// so the device only has to produce those counts, in one pass per pair of images:
//   area_gt[i], area_pred[j], tp[i][j]     label areas and the joint histogram
//   bnd_gt[i], bnd_pred[j]                 pixels of seg2bmap(gt == i), seg2bmap(pred == j)
//   fgm[i][j], gtm[i][j]                   the two true-positive counts of boundary_overlap(pred == j, gt == i)
// over the non-zero labels compacted to dense indices in ascending label order (np.unique minus the background).
//
// Structure of the boundary maps: seg2bmap(M) at pixel q compares M(q) with its right, lower and lower-right neighbours (the
// last row only with the right one, the last column only with the lower one, the bottom-right corner never).  For a label
// image, the labels whose boundary holds q are therefore the distinct labels of q's (reduced) 2x2 block when that block is
// not uniform.  Per pixel that set is a 64-bit mask over one 64-label chunk of each side; the dilation with disk(r) is an OR
// of the masks over the disk, read from an LDS tile with an r-pixel halo (pixels outside the image contribute nothing:
// cv2.dilate's default border).  Only boundary pixels (a few percent) do pair updates.  More than 64 labels on a side: the
// pass runs once per pair of 64-label chunks (grid z), same code.
//
// Kernels: zero -> per-image histograms (LDS tables, wave-uniform fast path) -> compaction (one workgroup per image, block
// scan) -> pair counts (16 x 64 pixel tiles).  Every result is an exact int32 count.
#include "common.h"

namespace {

constexpr int EV_BINS = 1024;                 // label values [0, 1024): LABEL_BINS of two_stage.py
constexpr int EV_HDR = 8;                     // per-image header of the counts row
constexpr int EV_TW = 64, EV_TH = 16, EV_THREADS = 256;
constexpr int EV_MAX_R = 16;

__host__ __device__ inline int64_t ev_row(int L) { return EV_HDR + 6 * (int64_t)L + 3 * (int64_t)L * L; }

// a float label value -> its bin; `bad` when it is not an integer in [0, EV_BINS) (counted, mapped to the background)
__device__ __forceinline__ int ev_bin(float f, bool& bad) {
    bad = !(f >= 0.f && f < (float)EV_BINS) || f != floorf(f);
    return bad ? 0 : (int)f;
}

__global__ void eval_zero_kernel(int* __restrict__ a, int64_t n, int* __restrict__ b, int64_t m) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n + m; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < n) a[i] = 0;
        else b[i - n] = 0;
    }
}

// hist [B][2][EV_BINS] (0: gt, 1: pred); header [2] / [3] of the counts row: invalid gt / pred pixels
__global__ __launch_bounds__(EV_THREADS) void eval_hist_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                               int* __restrict__ hist, int* __restrict__ counts, int64_t row, int n) {
    __shared__ int tab[2 * EV_BINS];
    __shared__ int over[2];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < 2 * EV_BINS; i += EV_THREADS) tab[i] = 0;
    if (threadIdx.x < 2) over[threadIdx.x] = 0;
    __syncthreads();
    const float* src[2] = {gt + (size_t)b * n, pred + (size_t)b * n};
    const int per = (n + gridDim.x - 1) / gridDim.x;
    const int p0 = blockIdx.x * per, p1 = min(n, p0 + per);
    const int lane = threadIdx.x & 63;
    for (int base = p0 + (threadIdx.x & ~63); base < p1; base += EV_THREADS) {      // wave-uniform trip count
        const int p = base + lane;
        const bool valid = p < p1;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            int v = 0;
            if (valid) {
                bool bad;
                v = ev_bin(src[s][p], bad);
                if (bad) atomicAdd(&over[s], 1);
            }
            const int v0 = __builtin_amdgcn_readfirstlane(v);
            const unsigned long long m = __ballot(valid), same = __ballot(valid && v == v0);
            if (same == m) {
                if (lane == 0) atomicAdd(&tab[s * EV_BINS + v0], __popcll(m));
            } else if (valid) {
                atomicAdd(&tab[s * EV_BINS + v], 1);
            }
        }
    }
    __syncthreads();
    int* h = hist + (size_t)b * 2 * EV_BINS;
    for (int i = threadIdx.x; i < 2 * EV_BINS; i += EV_THREADS)
        if (tab[i]) atomicAdd(h + i, tab[i]);
    if (threadIdx.x < 2 && over[threadIdx.x]) atomicAdd(counts + (size_t)b * row + 2 + threadIdx.x, over[threadIdx.x]);
}

// one workgroup of EV_BINS threads per image: dense index of every present non-zero label (ascending), map [B][2][EV_BINS]
// (-1 for absent labels and the background), header [0] / [1] = label counts, [4] / [5] = non-zero pixels of gt / pred,
// lab_* / area_* of the first L labels
__global__ __launch_bounds__(EV_BINS) void eval_compact_kernel(const int* __restrict__ hist, int* __restrict__ map,
                                                               int* __restrict__ counts, int64_t row, int L) {
    __shared__ int wsum[EV_BINS / 64];
    __shared__ int nz[2];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    int* c = counts + (size_t)b * row;
    if (t < 2) nz[t] = 0;
    __syncthreads();
    for (int s = 0; s < 2; ++s) {
        const int a = hist[((size_t)b * 2 + s) * EV_BINS + t];
        const bool present = a > 0 && t > 0;
        const unsigned long long bal = __ballot(present);
        if (lane == 0) wsum[w] = __popcll(bal);
        if (present) atomicAdd(&nz[s], a);
        __syncthreads();
        int off = 0;
        for (int k = 0; k < w; ++k) off += wsum[k];
        const int idx = off + __popcll(bal & ((1ull << lane) - 1ull));
        map[((size_t)b * 2 + s) * EV_BINS + t] = present ? idx : -1;
        if (present && idx < L) {
            c[EV_HDR + s * L + idx] = t;                   // lab_gt / lab_pred
            c[EV_HDR + (2 + s) * L + idx] = a;             // area_gt / area_pred
        }
        if (t == EV_BINS - 1) {
            int tot = 0;
            for (int k = 0; k < EV_BINS / 64; ++k) tot += wsum[k];
            c[s] = tot;
        }
        __syncthreads();
    }
    if (t < 2) c[4 + t] = nz[t];
}

__device__ __forceinline__ unsigned long long ev_bit(int v, int c0, int cn) {
    return (v >= c0 && v < c0 + cn) ? (1ull << (v - c0)) : 0ull;
}

// grid (ceil(W/64), ceil(H/16), B * NW * NW): one 16 x 64 tile of one image for one pair (gt chunk, pred chunk) of 64 labels
__global__ __launch_bounds__(EV_THREADS) void eval_pairs_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                const int* __restrict__ map, int* __restrict__ counts,
                                                                int64_t row, int H, int W, int R, int L, int NW) {
    extern __shared__ unsigned long long ev_smem[];
    const int z = blockIdx.z, b = z / (NW * NW), cw = z - b * NW * NW, cg = cw / NW, cp = cw - cg * NW;
    int* c = counts + (size_t)b * row;
    const int ng = min(c[0], L), np = min(c[1], L);
    const int g0 = cg * 64, p0 = cp * 64;
    if ((cg > 0 && g0 >= ng) || (cp > 0 && p0 >= np) || (ng == 0 && np == 0)) return;   // workgroup-uniform
    const int gc = max(0, min(64, ng - g0)), pc = max(0, min(64, np - p0));
    const int MW = EV_TW + 2 * R, MH = EV_TH + 2 * R, EW = MW + 1, EH = MH + 1;
    unsigned long long* mg = ev_smem;                                   // [MH][MW] boundary-label masks, gt chunk
    unsigned long long* mp = mg + MH * MW;                              // pred chunk
    int* tpl = reinterpret_cast<int*>(mp + MH * MW);                    // [64][64] joint counts of the chunk pair
    int* bndl = tpl + 64 * 64;                                          // [2][64] boundary pixels per label
    short* ig = reinterpret_cast<short*>(bndl + 128);                   // [EH][EW] dense gt index (-1 background, -2 outside)
    short* ip = ig + EH * EW;
    const int x0 = blockIdx.x * EV_TW, y0 = blockIdx.y * EV_TH;
    const int ex0 = x0 - R, ey0 = y0 - R;
    const int* mapg = map + (size_t)b * 2 * EV_BINS;
    const int* mapp = mapg + EV_BINS;
    const size_t plane = (size_t)H * W;
    const float* gimg = gt + (size_t)b * plane;
    const float* pimg = pred + (size_t)b * plane;

    for (int i = threadIdx.x; i < 64 * 64 + 128; i += EV_THREADS) tpl[i] = 0;
    for (int t = threadIdx.x; t < EH * EW; t += EV_THREADS) {
        const int ey = t / EW, ex = t - ey * EW, y = ey0 + ey, x = ex0 + ex;
        short a = -2, q = -2;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            bool bad;
            a = (short)mapg[ev_bin(gimg[(size_t)y * W + x], bad)];
            q = (short)mapp[ev_bin(pimg[(size_t)y * W + x], bad)];
        }
        ig[t] = a;
        ip[t] = q;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < MH * MW; t += EV_THREADS) {
        const int my = t / MW, mx = t - my * MW, y = ey0 + my, x = ex0 + mx;
        unsigned long long bg = 0, bp = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const bool hasE = x + 1 < W, hasS = y + 1 < H;
            const int o = my * EW + mx;
            {
                const int a = ig[o], e = hasE ? ig[o + 1] : a, s = hasS ? ig[o + EW] : a, se = (hasE && hasS) ? ig[o + EW + 1] : a;
                if (a != e || a != s || a != se) bg = ev_bit(a, g0, gc) | ev_bit(e, g0, gc) | ev_bit(s, g0, gc) | ev_bit(se, g0, gc);
            }
            {
                const int a = ip[o], e = hasE ? ip[o + 1] : a, s = hasS ? ip[o + EW] : a, se = (hasE && hasS) ? ip[o + EW + 1] : a;
                if (a != e || a != s || a != se) bp = ev_bit(a, p0, pc) | ev_bit(e, p0, pc) | ev_bit(s, p0, pc) | ev_bit(se, p0, pc);
            }
        }
        mg[t] = bg;
        mp[t] = bp;
    }
    __syncthreads();
    int* fgm = c + EV_HDR + 6 * L + L * L;
    int* gtm = fgm + L * L;
    const int lane = threadIdx.x & 63;
    for (int ty = threadIdx.x >> 6; ty < EV_TH; ty += EV_THREADS / 64) {   // wave-uniform: one tile row per wave
        const int y = y0 + ty, x = x0 + lane;
        const bool valid = y < H && x < W;
        const int my = ty + R, mx = lane + R;
        const int gi = ig[my * EW + mx], pj = ip[my * EW + mx];
        const int key = (valid && gi >= g0 && gi < g0 + gc && pj >= p0 && pj < p0 + pc) ? (gi - g0) * 64 + (pj - p0) : -1;
        const int k0 = __builtin_amdgcn_readfirstlane(key);
        const unsigned long long m = __ballot(valid), same = __ballot(valid && key == k0);
        if (same == m) {
            if (lane == 0 && k0 >= 0) atomicAdd(&tpl[k0], __popcll(m));
        } else if (key >= 0) {
            atomicAdd(&tpl[key], 1);
        }
        const unsigned long long Gq = valid ? mg[my * MW + mx] : 0ull, Pq = valid ? mp[my * MW + mx] : 0ull;
        if (Gq | Pq) {
            unsigned long long Gd = 0, Pd = 0;
            for (int dy = -R; dy <= R; ++dy) {
                int hw = R;
                while (hw * hw + dy * dy > R * R) --hw;                // disk(R): dx^2 + dy^2 <= R^2
                const unsigned long long* rg = mg + (my + dy) * MW + mx;
                const unsigned long long* rp = mp + (my + dy) * MW + mx;
                for (int dx = -hw; dx <= hw; ++dx) {
                    Gd |= rg[dx];
                    Pd |= rp[dx];
                }
            }
            if (cg == 0)
                for (unsigned long long r = Pq; r; r &= r - 1) atomicAdd(&bndl[64 + __builtin_ctzll(r)], 1);
            if (cp == 0)
                for (unsigned long long r = Gq; r; r &= r - 1) atomicAdd(&bndl[__builtin_ctzll(r)], 1);
            // fg_match: boundary pixels of pred j inside the dilated boundary of gt i; gt_match: the same with the sides swapped
            for (unsigned long long ri = Gd; ri; ri &= ri - 1) {
                const int i = g0 + __builtin_ctzll(ri);
                for (unsigned long long rj = Pq; rj; rj &= rj - 1) atomicAdd(fgm + (size_t)i * L + p0 + __builtin_ctzll(rj), 1);
            }
            for (unsigned long long ri = Gq; ri; ri &= ri - 1) {
                const int i = g0 + __builtin_ctzll(ri);
                for (unsigned long long rj = Pd; rj; rj &= rj - 1) atomicAdd(gtm + (size_t)i * L + p0 + __builtin_ctzll(rj), 1);
            }
        }
    }
    __syncthreads();
    int* tp = c + EV_HDR + 6 * L;
    for (int t = threadIdx.x; t < gc * pc; t += EV_THREADS) {
        const int i = t / pc, j = t - i * pc;
        const int v = tpl[i * 64 + j];
        if (v) atomicAdd(tp + (size_t)(g0 + i) * L + p0 + j, v);
    }
    if (threadIdx.x < 64) {
        const int t = threadIdx.x;
        if (cp == 0 && t < gc && bndl[t]) atomicAdd(c + EV_HDR + 4 * L + g0 + t, bndl[t]);
        if (cg == 0 && t < pc && bndl[64 + t]) atomicAdd(c + EV_HDR + 5 * L + p0 + t, bndl[64 + t]);
    }
}

size_t ev_pairs_lds(int R) {
    const int MW = EV_TW + 2 * R, MH = EV_TH + 2 * R;
    return (size_t)MH * MW * 16 + (64 * 64 + 128) * sizeof(int) + (size_t)(MH + 1) * (MW + 1) * 2 * sizeof(short);
}

}  // namespace

extern "C" int64_t msm_eval_counts_workspace(int B) {
    return B < 0 ? -1 : (int64_t)B * 4 * EV_BINS * (int64_t)sizeof(int32_t);
}

extern "C" int msm_eval_counts(const float* pred, const float* gt, int32_t* counts, void* workspace, int64_t workspace_bytes,
                               int B, int H, int W, int radius, int L, void* stream) {
    MSM_REQUIRE(pred && gt && counts && workspace, "msm_eval_counts: null pointer");
    MSM_REQUIRE(B >= 0 && H > 0 && W > 0 && (int64_t)H * W < (1 << 30), "msm_eval_counts: bad shape B=%d H=%d W=%d", B, H, W);
    MSM_REQUIRE(radius >= 0 && radius <= EV_MAX_R, "msm_eval_counts: radius %d outside [0, %d]", radius, EV_MAX_R);
    MSM_REQUIRE(L >= 1 && L <= EV_BINS, "msm_eval_counts: L=%d outside [1, %d]", L, EV_BINS);
    MSM_REQUIRE(workspace_bytes >= msm_eval_counts_workspace(B), "msm_eval_counts: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)msm_eval_counts_workspace(B));
    if (B == 0) return MSM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t row = ev_row(L);
    int* hist = static_cast<int*>(workspace);
    int* map = hist + (size_t)B * 2 * EV_BINS;
    const int64_t nz = (int64_t)B * row, nh = (int64_t)B * 2 * EV_BINS;
    const int NW = (L + 63) / 64;
    MSM_REQUIRE((int64_t)B * NW * NW <= 65535, "msm_eval_counts: B * ceil(L/64)^2 = %lld exceeds the grid", (long long)B * NW * NW);
    const int64_t zb = (nz + nh + 255) / 256;
    hipLaunchKernelGGL(eval_zero_kernel, dim3((unsigned)(zb < 1024 ? zb : 1024)), dim3(256), 0, s, counts, nz, hist, nh);
    const int n = H * W;
    int gx = msm::cdiv(n, EV_THREADS * 16);
    gx = max(1, min(gx, max(1, 1024 / B)));
    hipLaunchKernelGGL(eval_hist_kernel, dim3(gx, B), dim3(EV_THREADS), 0, s, pred, gt, hist, counts, row, n);
    hipLaunchKernelGGL(eval_compact_kernel, dim3(B), dim3(EV_BINS), 0, s, hist, map, counts, row, L);
    const size_t lds = ev_pairs_lds(radius);
    MSM_CHECK_HIP((hipError_t)msm::ensure_dynamic_lds((const void*)eval_pairs_kernel, lds));
    hipLaunchKernelGGL(eval_pairs_kernel, dim3(msm::cdiv(W, EV_TW), msm::cdiv(H, EV_TH), B * NW * NW), dim3(EV_THREADS), lds, s, pred, gt,
                       map, counts, row, H, W, radius, L, NW);
    MSM_CHECK_LAUNCH("msm_eval_counts");
    return MSM_OK;
}
