// Mask NMS for a batch of images: combine_masks_with_NMS (lib/fcn/test_utils.py:55-91) over nms (lib/fcn/nms.py:3-23), the
// "real world images" configuration of the reference (USE_NMS, test_utils.py:30), with fixed shapes and no host synchronisation.
//
// The reference forms an N x N intersection matrix with one numpy product per pair over the full-resolution float masks, loops
// greedily in Python and paints the survivors into a label image.  Here:
//   pack      candidate masks -> bit planes (one 64-bit word per 64 consecutive pixels of the flattened image, built with wave
//             ballots) + area and tight box per mask (integer atomics).  Non-candidate planes are never read.
//   pairs     inter[i][j] = popcount(plane_i & plane_j) for candidate pairs i < j: 1/32 of the float traffic per operand, exact.
//   select    one workgroup per image: visiting order, greedy suppression, area ranking, boxes (K <= 256).
//   compose   label and score images from the bit planes of the kept masks.
// Every count is an integer sum, so no result depends on the grid size or on the order of the atomics; the only floating-point
// operation that decides anything is the one correctly rounded fp32 division of the IoU.  The definition is in include/msm_hip.h.
#include "common.h"

namespace {

constexpr int NMS_THREADS = 256;
constexpr int NMS_WAVES = NMS_THREADS / 64;
constexpr int NMS_MAX_K = 256;                 // select: one thread per instance
constexpr int PACK_UNROLL = 4;                 // pack: words per wave and trip (independent loads in flight)
constexpr int PAIR_REGS = 4;                   // pairs: words of the row's plane a lane keeps in registers
constexpr int PAIR_CHUNK = 64 * PAIR_REGS;     // words of every plane one workgroup of the pairs kernel covers

typedef unsigned long long u64;

struct Layout {                                // byte offsets into the workspace
    int64_t nw;                                // words per plane
    size_t bits, inter, area, ext, sval, total;
};

inline Layout layout(int B, int K, int H, int W) {
    Layout L;
    L.nw = ((int64_t)H * W + 63) / 64;
    const size_t bk = (size_t)B * K;
    size_t o = 0;
    L.bits = o;  o += bk * (size_t)L.nw * sizeof(u64);
    L.inter = o; o += bk * K * sizeof(int32_t);  o = (o + 15) & ~(size_t)15;
    L.area = o;  o += bk * sizeof(int32_t);      o = (o + 15) & ~(size_t)15;
    L.ext = o;   o += bk * 4 * sizeof(int32_t);
    L.sval = o;  o += bk * sizeof(float);        o = (o + 15) & ~(size_t)15;
    L.total = o;
    return L;
}

// the get_confident_instances flag, minus NaN scores (they have no place in the visiting order)
__device__ __forceinline__ bool is_candidate(const uint8_t* __restrict__ cand, const float* __restrict__ scores, int64_t i) {
    const float s = scores[i];
    return cand[i] != 0 && s == s;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ void nms_init_kernel(int32_t* __restrict__ inter, int32_t* __restrict__ area, int32_t* __restrict__ ext, int64_t n_inter,
                                int64_t n_area, int H, int W) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_inter; i += step) inter[i] = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_area; i += step) {
        area[i] = 0;
        int32_t* e = ext + i * 4;
        e[0] = W; e[1] = H; e[2] = -1; e[3] = -1;
    }
}

// grid (gx, K, B): workgroup (x, k, b) packs words x*4 + wave, stepping by gridDim.x * 4 quadruples, of plane (b, k)
__global__ __launch_bounds__(NMS_THREADS) void nms_pack_kernel(const float* __restrict__ masks, const float* __restrict__ scores,
                                                               const uint8_t* __restrict__ cand, u64* __restrict__ bits,
                                                               int32_t* __restrict__ area, int32_t* __restrict__ ext, int K, int n, int H,
                                                               int W, int64_t nw) {
    const int64_t bk = (int64_t)blockIdx.z * K + blockIdx.y;
    if (!is_candidate(cand, scores, bk)) return;                    // before any float of the plane is read
    const float* m = masks + bk * n;
    u64* out = bits + bk * nw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int cnt = 0, xmin = W, ymin = H, xmax = -1, ymax = -1;
    for (int64_t w0 = ((int64_t)blockIdx.x * NMS_WAVES + wave) * PACK_UNROLL; w0 < nw; w0 += (int64_t)gridDim.x * NMS_WAVES * PACK_UNROLL) {
        float v[PACK_UNROLL];
#pragma unroll
        for (int j = 0; j < PACK_UNROLL; ++j) {
            const int64_t p = (w0 + j) * 64 + lane;
            v[j] = p < n ? m[p] : 0.f;                               // past the image: outside (masks the last word)
        }
#pragma unroll
        for (int j = 0; j < PACK_UNROLL; ++j) {
            const bool in = v[j] != 0.f;
            const u64 word = __ballot(in);
            if (w0 + j < nw) {
                if (lane == 0) out[w0 + j] = word;
                cnt += __popcll(word);
                if (in) {
                    const int p = (int)((w0 + j) * 64) + lane;
                    const int y = p / W, x = p - y * W;
                    xmin = min(xmin, x); ymin = min(ymin, y); xmax = max(xmax, x); ymax = max(ymax, y);
                }
            }
        }
    }
    if (cnt == 0) return;                                            // wave-uniform
    xmin = wave_min_int(xmin); ymin = wave_min_int(ymin); xmax = wave_max_int(xmax); ymax = wave_max_int(ymax);
    if (lane == 0) {
        atomicAdd(area + bk, cnt);
        int32_t* e = ext + bk * 4;
        atomicMin(e, xmin); atomicMin(e + 1, ymin); atomicMax(e + 2, xmax); atomicMax(e + 3, ymax);
    }
}

// grid (chunks, B): workgroup (c, b) covers words [c * PAIR_CHUNK, (c + 1) * PAIR_CHUNK) of every candidate plane of image b.  Wave v takes
// the rows a = v, v + 4, ... of the candidate list: the row's words stay in registers while the planes after it stream past; the
// partial count of a pair is summed over the wave and added once to inter[i][j] (i < j: the upper triangle).
__global__ __launch_bounds__(NMS_THREADS) void nms_pairs_kernel(const u64* __restrict__ bits, const float* __restrict__ scores,
                                                                const uint8_t* __restrict__ cand, int32_t* __restrict__ inter, int K,
                                                                int64_t nw) {
    __shared__ int list[NMS_MAX_K];
    __shared__ int wave_count[NMS_WAVES];
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t bK = (int64_t)b * K;
    const bool c = t < K && is_candidate(cand, scores, bK + t);
    const u64 bal = __ballot(c);
    if (lane == 0) wave_count[wave] = __popcll(bal);
    __syncthreads();
    int off = 0, nc = 0;
#pragma unroll
    for (int i = 0; i < NMS_WAVES; ++i) {
        if (i < wave) off += wave_count[i];
        nc += wave_count[i];
    }
    if (c) list[off + __popcll(bal & ((1ull << lane) - 1ull))] = t;  // ascending index order
    __syncthreads();
    if (nc < 2) return;
    const int64_t w0 = (int64_t)blockIdx.x * PAIR_CHUNK + lane;
    for (int a = wave; a < nc - 1; a += NMS_WAVES) {
        const int i = list[a];
        const u64* pi = bits + (bK + i) * nw;
        u64 wi[PAIR_REGS], any = 0;
#pragma unroll
        for (int r = 0; r < PAIR_REGS; ++r) {
            const int64_t w = w0 + r * 64;
            wi[r] = w < nw ? pi[w] : 0ull;
            any |= wi[r];
        }
        if (__ballot(any != 0ull) == 0ull) continue;                 // the row's mask has no pixel in this chunk
        for (int a2 = a + 1; a2 < nc; ++a2) {
            const int j = list[a2];
            const u64* pj = bits + (bK + j) * nw;
            int s = 0;
#pragma unroll
            for (int r = 0; r < PAIR_REGS; ++r) {
                const int64_t w = w0 + r * 64;
                if (w < nw) s += __popcll(wi[r] & pj[w]);
            }
            s = wave_sum_int(s);
            if (lane == 0 && s != 0) atomicAdd(inter + (bK + i) * K + j, s);
        }
    }
}

// one workgroup per image, thread t = instance t
__global__ __launch_bounds__(NMS_THREADS) void nms_select_kernel(const float* __restrict__ scores, const uint8_t* __restrict__ cand,
                                                                 const int32_t* __restrict__ area, const int32_t* __restrict__ ext,
                                                                 int32_t* __restrict__ inter, float* __restrict__ sval,
                                                                 int32_t* __restrict__ inst_labels, float* __restrict__ bbox,
                                                                 int32_t* __restrict__ count, int K, float thresh) {
    __shared__ float s_score[NMS_MAX_K];
    __shared__ int s_area[NMS_MAX_K], s_cand[NMS_MAX_K], s_valid[NMS_MAX_K], s_alive[NMS_MAX_K], s_order[NMS_MAX_K], s_kept[NMS_MAX_K];
    __shared__ int s_nk;
    const int b = blockIdx.x, t = threadIdx.x;
    const int64_t bK = (int64_t)b * K;
    float sc = 0.f;
    int ar = 0;
    bool c = false;
    if (t < K) {
        sc = scores[bK + t];
        c = is_candidate(cand, scores, bK + t);
        ar = c ? area[bK + t] : 0;
    }
    const bool valid = c && ar > 0;                                  // an empty candidate is dropped before NMS
    s_score[t] = sc; s_area[t] = ar; s_cand[t] = c; s_valid[t] = valid; s_alive[t] = valid; s_kept[t] = -1;
    __syncthreads();
    // the full matrix for whoever reads the workspace: area on the diagonal, the upper triangle mirrored
    int32_t* mat = inter + bK * K;
    for (int idx = t; idx < K * K; idx += NMS_THREADS) {
        const int i = idx / K, j = idx - i * K;
        if (!s_cand[i] || !s_cand[j]) continue;
        if (i == j) mat[idx] = s_area[i];
        else if (i > j) mat[idx] = mat[(int64_t)j * K + i];
    }
    // visiting order: descending score, equal scores the higher index first
    int rank = 0;
    if (valid) {
        for (int u = 0; u < K; ++u) {
            const float su = s_score[u];
            if (s_valid[u] && (su > sc || (su == sc && u > t))) ++rank;
        }
        s_order[rank] = t;
    }
    const int nc = __syncthreads_count(valid);
    // greedy suppression
    int nk = 0;                                                      // thread 0's count of kept instances
    for (int p = 0; p < nc; ++p) {
        const int i = s_order[p];
        if (!s_alive[i]) continue;                                   // uniform: nobody writes s_alive[i] in or after trip rank(i)
        if (t == 0) s_kept[i] = nk++;
        if (valid && rank > p && s_alive[t]) {
            const int in = i < t ? mat[(int64_t)i * K + t] : mat[(int64_t)t * K + i];
            const float iou = (float)in / (float)(s_area[i] + ar - in);
            if (!(iou <= thresh)) s_alive[t] = 0;                    // a NaN quotient suppresses
        }
        __syncthreads();
    }
    if (t == 0) s_nk = nk;
    __syncthreads();
    nk = s_nk;
    // kept instances by area ascending, equal areas in the order they were kept: rank r carries label 2 + r
    const int mine = s_kept[t];
    int r = 0;
    if (mine >= 0) {
        for (int u = 0; u < K; ++u) {
            const int ku = s_kept[u];
            if (ku >= 0 && (s_area[u] < ar || (s_area[u] == ar && ku < mine))) ++r;
        }
        float* row = bbox + (bK + r) * 5;
        const int32_t* e = ext + (bK + t) * 4;
        row[0] = (float)e[0]; row[1] = (float)e[1]; row[2] = (float)e[2]; row[3] = (float)e[3]; row[4] = sc;
    }
    if (t < K) {
        inst_labels[bK + t] = mine >= 0 ? 2 + r : 0;
        sval[bK + t] = mine >= 0 ? truncf(sc * 100.f) : 0.f;
        if (t >= nk) {
            float* row = bbox + (bK + t) * 5;
            row[0] = 0.f; row[1] = 0.f; row[2] = 0.f; row[3] = 0.f; row[4] = 0.f;
        }
    }
    if (t == 0) count[b] = nk;
}

// grid (gx, B): a wave paints 64 consecutive pixels per trip from one word of every kept plane, largest label first
__global__ __launch_bounds__(NMS_THREADS) void nms_compose_kernel(const u64* __restrict__ bits, const int32_t* __restrict__ inst_labels,
                                                                  const float* __restrict__ sval, const int32_t* __restrict__ count,
                                                                  float* __restrict__ label, float* __restrict__ score_img, int K, int n,
                                                                  int64_t nw) {
    __shared__ int s_k[NMS_MAX_K];
    __shared__ float s_sv[NMS_MAX_K];
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t bK = (int64_t)b * K;
    const int nk = count[b];
    if (t < K) {
        const int l = inst_labels[bK + t];
        if (l >= 2) { s_k[l - 2] = t; s_sv[l - 2] = sval[bK + t]; }
    }
    __syncthreads();
    for (int64_t w = (int64_t)blockIdx.x * NMS_WAVES + wave; w < nw; w += (int64_t)gridDim.x * NMS_WAVES) {
        const int64_t p = w * 64 + lane;
        float lab = 0.f, sv = 0.f;
        for (int r = nk - 1; r >= 0; --r) {
            const u64 word = bits[(bK + s_k[r]) * nw + w];
            if (lab == 0.f && ((word >> lane) & 1ull)) { lab = (float)(r + 2); sv = s_sv[r]; }
            if (__ballot(lab == 0.f) == 0ull) break;
        }
        if (p < n) {
            label[(int64_t)b * n + p] = lab;
            score_img[(int64_t)b * n + p] = sv;
        }
    }
}

bool shape_ok(int B, int K, int H, int W) {
    return B > 0 && B <= 65535 && K > 0 && K <= NMS_MAX_K && H > 0 && W > 0 && (int64_t)H * W <= (1 << 24);
}

}  // namespace

extern "C" int64_t msm_mask_nms_workspace(int B, int K, int H, int W) {
    if (!shape_ok(B, K, H, W)) {
        msm::set_error("msm_mask_nms_workspace: B=%d K=%d H=%d W=%d outside 0 < B <= 65535, 0 < K <= %d, 0 < H*W <= 2^24", B, K, H, W, NMS_MAX_K);
        return MSM_E_INVALID;
    }
    return (int64_t)layout(B, K, H, W).total;
}

extern "C" int msm_mask_nms(const float* masks, const float* scores, const uint8_t* candidate, float thresh, float* label, float* score_img,
                            float* bbox, int32_t* count, int32_t* inst_labels, void* workspace, int64_t workspace_bytes, int B, int K,
                            int H, int W, void* stream) {
    MSM_REQUIRE(shape_ok(B, K, H, W), "msm_mask_nms: B=%d K=%d H=%d W=%d outside 0 < B <= 65535, 0 < K <= %d (one select thread per instance), 0 < H*W <= 2^24",
                B, K, H, W, NMS_MAX_K);
    MSM_REQUIRE(masks && scores && candidate && label && score_img && bbox && count && inst_labels && workspace, "msm_mask_nms: null pointer");
    MSM_REQUIRE((((uintptr_t)workspace) & 15) == 0, "msm_mask_nms: the workspace must be 16-byte aligned");
    const Layout L = layout(B, K, H, W);
    if (workspace_bytes < (int64_t)L.total) {
        msm::set_error("msm_mask_nms: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.total);
        return MSM_E_WORKSPACE;
    }
    char* ws = (char*)workspace;
    u64* bits = (u64*)(ws + L.bits);
    int32_t* inter = (int32_t*)(ws + L.inter);
    int32_t* area = (int32_t*)(ws + L.area);
    int32_t* ext = (int32_t*)(ws + L.ext);
    float* sval = (float*)(ws + L.sval);
    hipStream_t s = (hipStream_t)stream;
    const int n = H * W;
    const int64_t n_area = (int64_t)B * K, n_inter = n_area * K;
    hipLaunchKernelGGL(nms_init_kernel, dim3((unsigned)min((int64_t)1024, (n_inter + 255) / 256)), dim3(256), 0, s, inter, area, ext, n_inter,
                       n_area, H, W);
    const int gx = max(1, min(16, msm::cdiv(L.nw, NMS_WAVES * PACK_UNROLL * 4)));
    hipLaunchKernelGGL(nms_pack_kernel, dim3(gx, K, B), dim3(NMS_THREADS), 0, s, masks, scores, candidate, bits, area, ext, K, n, H, W, L.nw);
    hipLaunchKernelGGL(nms_pairs_kernel, dim3(msm::cdiv(L.nw, PAIR_CHUNK), B), dim3(NMS_THREADS), 0, s, bits, scores, candidate, inter, K, L.nw);
    hipLaunchKernelGGL(nms_select_kernel, dim3(B), dim3(NMS_THREADS), 0, s, scores, candidate, area, ext, inter, sval, inst_labels, bbox, count,
                       K, thresh);
    const int gc = max(1, min(msm::cdiv(L.nw, NMS_WAVES * 4), max(1, 2048 / B)));
    hipLaunchKernelGGL(nms_compose_kernel, dim3(gc, B), dim3(NMS_THREADS), 0, s, bits, inst_labels, sval, count, label, score_img, K, n, L.nw);
    MSM_CHECK_LAUNCH("msm_mask_nms");
    return MSM_OK;
}
